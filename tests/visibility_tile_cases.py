"""Inputs that make the three readers of a finished visibility buffer — orbit_visibility_resolve, the mark launch of
orbit_visibility_compact, orbit_visibility_surface — run their tile loop MORE THAN ONCE per wave, with something else in
every trip, and lists that make the compaction's totals launch run its loop a second time.  As in the
sibling case files the expected bytes are never computed here: the GPU tests' reference is the host mirror
(orbit_amd.raster.host_visibility_*), which tests/test_visibility_tiles_cpu.py holds to the numpy restatements; a case
states only counters known in closed form (`expect`).

One tile programme, three readers.  A target is cut into 8 x 8 pixel tiles, tile = ty * tiles_x + tx, and every tile is
given a KIND:
  E        empty
  O        one key on all 64 pixels: one command, one triangle over the tile.  `O:r<t>` is triangle t of the RING, one
           command of 34 triangles (all but the named ones without area) that owns several tiles
  K        64 distinct keys: 64 commands with one single-pixel triangle each
  F        covered, but only by ids outside [base, base + n): base - 1 and base + n in turn, written by hand
  M        owned, foreign and uncovered pixels mixed: a command of two keys (a 4 x 4 square), one of one key (6 pixels),
           three foreign pixels written by hand
  Px       owned pixels only, one single-pixel triangle per pixel of the tile's first column: the partial column's tile
  Py       owned pixels only, one triangle of the entity whose w is 2^-100, 30 000 pixels wide with corner 1 at the
           tile: the partial row's tile.  1 / w times an edge value overflows there, so every pixel is also degenerate
  S:<way>  (surface) the tile's one command fails R9 by <way> — corner (a corner byte = vcount), index (an index word
           beyond vertex_count), entity (cmd_first_instance = entity_count) —, the raster skips it, and a word naming it is
           written by hand into all 64 pixels.  For the resolve the command is owned; for the compaction it is visible
  SG       such a command on the tile's lower half and a good one (a 4 x 4 square) on its upper half
  X        (surface) a triangle cut by the near plane, drawn with ORBIT_RASTER_CLIP_NEAR: unsupported
  W        the tile's first pixel row, owned by the SAME key in every W tile of the programme: one triangle of one command,
           half a pixel high and as wide as the target, at a depth (0.2) behind everything else, so that it is left only
           where its tile holds nothing else.  The W tiles lie in one tile row
A programme is drawn by host_raster_visibility (pixel_proj, CLIP_NEAR, command_base = BASE), every tile's content at the
depth 1/4 + tile / 128, so that what a triangle spills to the right of and below its tile loses against what is drawn
there; then it is tampered with by hand: a word whose key does not belong to its pixel's tile is set to 0 (the spill
into empty and partly covered tiles), and the F, M, S and SG words are written.

Which tiles a wave takes is a closed formula: with need = ceil(tiles / 4) workgroups and a cap of c (0: the resident
grid), the wave with global index g takes g, g + G, g + 2 G, ... with G = 4 * min(need, c).  arrangements() works from
the kinds and that formula alone and returns which of ARRANGEMENTS some wave meets:
  a:E>O a:O>E>O          an empty tile — the surface's uniform `continue` —, then work
  b:K>O>K                64 trips of the numbering loop, 1, 64: the numbering state and the setup lanes
  c:F>O c:F_alone        nothing owned, then work; F as a wave's only tile
  d:Px>full d:Py_last    8 lanes (or 1) store, then all 64 are needed again; a partial tile as the last of several
  e:<way>>O e:SG         a failed command's verdict, then a good command on the same lanes; both in one tile
  f:X>O                  unsupported, then written
  g:one_wave g:two_waves g:two_words   the ring owned in two tiles of one wave (the resolve counts the command visible
                         once), in tiles of two waves, and with triangles t and t + 32 — the same bit of two mask words
                         — in two trips of one wave
  g:own_bit              one key (the W triangle) owned in two tiles of one wave: in the later trip the mark's relaxed load
                         finds the bit that an earlier trip of the same wave set
  h:idle_wave            a wave without a tile beside one with
  i:<call>.<counter>     the counter receives a share from two trips of one wave and from two waves
The four targets of programmes() together hold all of them under a cap of 1 and of 2 workgroups.

Second-round lists (no raster; CHUNK = 256 commands per block of the scan, 256 block totals per round of the totals
launch): chunks_258, chunks_257_listed_short, chunks_512_exact — see second_round_cases()."""
from dataclasses import dataclass, field

import numpy as np

import raster_cases as rc
import raster_vis_cases as vc
import raster_walk_cases as wk
import visibility_compact_cases as cc
import visibility_surface_cases as sc
from raster_cases import poly
from raster_vis_cases import _word
from visibility_surface_cases import pixel_triangle

F = np.float32
WAVES = 4        # of a workgroup
RESIDENT = 2048  # workgroups of the uncapped grid on a 256-CU device (num_cus * 8)
BASE = 1000      # command_base of every programme
CAPS = (1, 2, 0)
CHUNK = cc.CHUNK
ROUND = 256      # block totals per round of compact_totals_kernel
S_WAYS = ("corner", "index", "entity")  # of S:<way> ...
S_FAULTS = dict(corner="corner_is_vcount", index="vertex_word", entity="entity_is_entity_count")  # ... in raster_walk_cases.FAULTS
TINY_W = np.ascontiguousarray((np.eye(4, dtype=F) * F(2.0) ** F(-100)).T.reshape(16))  # clip = 2^-100 * (x, y, z, 1)

# the counters a tile of a kind gives a non-zero share to, per call (OrbitVisibilityStats, the two counters of
# OrbitVisibilityCompactStats that the mark launch counts, OrbitSurfaceStats)
_OWNED = ("resolve.covered_pixels", "resolve.visible_commands", "compact.covered_pixels", "surface.covered_pixels")
_FOREIGN = ("resolve.covered_pixels", "resolve.foreign_pixels", "compact.covered_pixels", "compact.foreign_pixels",
            "surface.covered_pixels", "surface.foreign_pixels")
SHARES = {"E": (), "O": _OWNED + ("surface.written_pixels",), "K": _OWNED + ("surface.written_pixels",), "F": _FOREIGN,
          "M": _OWNED + _FOREIGN + ("surface.written_pixels",), "Px": _OWNED + ("surface.written_pixels",),
          "Py": _OWNED + ("surface.written_pixels", "surface.degenerate_pixels"), "S": _OWNED + ("surface.stale_pixels",),
          "SG": _OWNED + ("surface.written_pixels", "surface.stale_pixels"), "X": _OWNED + ("surface.unsupported_pixels",),
          "W": _OWNED + ("surface.written_pixels",)}
COUNTERS = tuple(sorted({c for v in SHARES.values() for c in v}))
ARRANGEMENTS = ("a:E>O", "a:O>E>O", "b:K>O>K", "c:F>O", "c:F_alone", "d:Px>full", "d:Py_last") + tuple(f"e:{w}>O" for w in S_WAYS) + \
    ("e:SG", "f:X>O", "g:one_wave", "g:two_waves", "g:two_words", "g:own_bit", "h:idle_wave") + tuple(f"i:{c}" for c in COUNTERS)


def base_kind(kind):
    return kind.split(":")[0]


def assignment(tiles, cap, resident=RESIDENT):
    """-> per wave of the grid the tiles it takes, in order: wave g takes g, g + G, ..., G = 4 * min(need, cap)"""
    need = (tiles + WAVES - 1) // WAVES
    waves = WAVES * min(need, cap if cap else resident, resident)
    return [list(range(g, tiles, waves)) for g in range(waves)]


def arrangements(kinds, tiles, cap, resident=RESIDENT):
    """What the assignment of `tiles` tiles of `kinds` to the waves of a grid capped at `cap` workgroups holds, of
    ARRANGEMENTS (the module's docstring); nothing is rasterised."""
    assert len(kinds) == tiles
    found, ring_waves = set(), set()
    waves = assignment(tiles, cap, resident)
    if any(not w for w in waves) and any(w for w in waves):
        found.add("h:idle_wave")
    sharing = {c: set() for c in COUNTERS}
    for g, w in enumerate(waves):
        seq = [kinds[t] for t in w]
        b = [base_kind(k) for k in seq]
        for i in range(len(b)):
            two, three = tuple(b[i:i + 2]), tuple(b[i:i + 3])
            if two == ("E", "O"):
                found.add("a:E>O")
            if three == ("O", "E", "O"):
                found.add("a:O>E>O")
            if three == ("K", "O", "K"):
                found.add("b:K>O>K")
            if two == ("F", "O"):
                found.add("c:F>O")
            if len(two) == 2 and two[0] == "Px" and two[1] in ("O", "K"):
                found.add("d:Px>full")
            if two == ("S", "O"):
                found.add(f"e:{seq[i].split(':')[1]}>O")
            if two == ("X", "O"):
                found.add("f:X>O")
        if b == ["F"]:
            found.add("c:F_alone")
        if len(b) > 1 and b[-1] == "Py":
            found.add("d:Py_last")
        if "SG" in b:
            found.add("e:SG")
        ring = [int(k.split(":r")[1]) for k in seq if k.startswith("O:r")]
        if len(ring) > 1:
            found.add("g:one_wave")
            if any(t + 32 in ring for t in ring):  # the same bit of two mask words
                found.add("g:two_words")
        if ring:
            ring_waves.add(g)
        if b.count("W") > 1:
            found.add("g:own_bit")
        for c in COUNTERS:
            trips = sum(1 for k in b if c in SHARES[k])
            if trips:
                sharing[c].add((g, trips > 1))
    if len(ring_waves) > 1:
        found.add("g:two_waves")
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
    visibility: np.ndarray = None   # (h, w) uint64: drawn, then tampered with
    packed: object = None           # rc.Packed of the list
    surface: object = None          # sc.SurfaceCase over them
    compact: object = None          # cc.CompactCase over them
    expect: dict = field(default_factory=dict)  # {call: {counter: value}}

    @property
    def tiles(self):
        return ((self.width + 7) // 8) * ((self.height + 7) // 8)

    @property
    def max_commands(self):
        return self.packed.max_commands


def depth_of(tile):
    return float(F(0.25) + F(tile) / F(128))


def _square(x, y, z):
    return [tuple((px, py, z) for px, py in t) for t in vc.tile(x, y, z)[0]]


def programme(name, width, height, kinds):
    tiles_x, tiles_y = (width + 7) // 8, (height + 7) // 8
    assert len(kinds) == tiles_x * tiles_y and width <= 80 and height <= 40
    flat = ((0.0, 0.0, 0.5),) * 3  # no area
    ring = {int(k.split(":r")[1]): t for t, k in enumerate(kinds) if k.startswith("O:r")}
    wide = [t for t, k in enumerate(kinds) if k == "W"]
    meshlets, owner, faults, by_hand = [], [], {}, []  # owner[k]: command k's tile (the ring: -1, the W triangle: -3)

    def add(tile, tris, entity=0):
        meshlets.append(poly(tris, entity=entity))
        owner.append(tile)
        return len(meshlets) - 1

    def over(x0, y0, z):  # one triangle over the whole tile at (x0, y0); it spills to the right and below
        return ((x0, y0, z), (x0, y0 + 16.5, z), (x0 + 16.5, y0, z))

    if ring:
        tris = [flat] * (max(ring) + 1)
        for t, tile in ring.items():
            tris[t] = over(8 * (tile % tiles_x), 8 * (tile // tiles_x), depth_of(tile))
        add(-1, tris)
    if wide:
        assert len({t // tiles_x for t in wide}) == 1
        y = 8 * (wide[0] // tiles_x)
        add(-3, [((0.25, y + 0.25, 0.2), (0.25, y + 0.75, 0.2), (3.0 * width, y + 0.5, 0.2))])
    for tile, kind in enumerate(kinds):
        x0, y0, z = 8 * (tile % tiles_x), 8 * (tile // tiles_x), depth_of(tile)
        pw, ph = min(8, width - x0), min(8, height - y0)  # the tile's pixels inside the target
        b = base_kind(kind)
        assert b in SHARES and (pw == ph == 8 or b in ("E", "Px", "Py", "F", "W")), (tile, kind)
        if kind == "O":
            add(tile, [over(x0, y0, z)])
        elif b == "K":
            for q in range(64):
                add(tile, [pixel_triangle(x0 + q % 8, y0 + q // 8, z)])
        elif b == "F":
            by_hand.append(("foreign", [(y0 + q // pw, x0 + q % pw) for q in range(pw * ph)]))
        elif b == "M":
            add(tile, _square(x0, y0, z))
            add(tile, [((x0 + 4.25, y0 + 4.25, z), (x0 + 4.25, y0 + 7.75, z), (x0 + 7.75, y0 + 4.25, z))])
            by_hand.append(("foreign", [(y0, x0 + 5), (y0 + 1, x0 + 6), (y0 + 2, x0 + 7)]))
        elif b == "Px":
            add(tile, [pixel_triangle(x0, y0 + q, z) for q in range(ph)])
        elif b == "Py":  # (corner 1 at the tile: the quotient that S3 divides by s is the one that overflows)
            add(tile, [((x0 + 30000.0, y0 + 0.25, z), (x0 + 0.25, y0 + 0.25, z), (x0 + 0.25, y0 + 30000.0, z))], entity=1)
        elif b in ("S", "SG"):
            k = add(tile, [((x0 + 1.0, y0 + 1.0, z), (x0 + 1.0, y0 + 6.0, z), (x0 + 6.0, y0 + 1.0, z))])
            faults[k] = S_FAULTS[kind.split(":")[1] if b == "S" else "corner"]
            if b == "SG":
                add(tile, _square(x0, y0, z))
            by_hand.append((k, [(y0 + q // 8, x0 + q % 8) for q in range(32 if b == "SG" else 0, 64)]))
        elif b == "X":  # its third vertex lies in front of the near plane z = w
            add(tile, [((x0 + 1.0, y0 + 1.0, z), (x0 + 1.0, y0 + 7.0, z), (x0 + 7.0, y0 + 1.0, 2.0))])
    n = len(meshlets)
    case = wk.WalkCase(name, meshlets, width=width, height=height, entities=[rc.IDENTITY, TINY_W], command_base=BASE,
                       clip_near=True, mutate=wk.write_faults(faults), faults=faults)
    pk = rc.Packed(case)
    vis, stats, errors = wk.host_vis(pk)
    assert sorted(np.flatnonzero(errors)) == sorted(faults) and int(stats["clip_skipped"]) == 0, name
    # by hand, 1: a key that does not belong to its pixel's tile (what a triangle spills beyond its tile) -> 0
    ys, xs = np.mgrid[0:height, 0:width]
    tile_of_pixel = (ys // 8) * tiles_x + xs // 8
    k = ((vis >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.int64) - BASE
    t = (vis & np.uint64(255)).astype(np.int64)
    assert ((vis == 0) | ((k >= 0) & (k < n))).all()
    tile_of_key = np.asarray(owner, np.int64)[np.clip(k, 0, max(n - 1, 0))] if n else np.full(vis.shape, -2)
    if ring:
        ring_tiles = np.full(256, -2, np.int64)
        ring_tiles[list(ring)] = list(ring.values())
        tile_of_key = np.where(tile_of_key == -1, ring_tiles[t], tile_of_key)
    if wide:
        tile_of_key = np.where((tile_of_key == -3) & np.isin(tile_of_pixel, wide), tile_of_pixel, tile_of_key)
    vis = np.where(tile_of_key == tile_of_pixel, vis, np.uint64(0))
    # by hand, 2: the foreign words and the words that name a command the raster skipped
    stale = []
    for what, pixels in by_hand:
        for q, (y, x) in enumerate(pixels):
            assert vis[y, x] == 0
            if what == "foreign":
                vis[y, x] = _word(F(0.5), BASE - 1 if (x + y) % 2 else BASE + n, q % 3)
            else:
                vis[y, x] = _word(F(0.5), BASE + what, 0)
                stale.append((y, x))
    count = lambda kind: sum(1 for q in kinds if base_kind(q) == kind)  # noqa: E731
    in_target = lambda kind, first_column=False: sum(  # noqa: E731
        (1 if first_column else min(8, width - 8 * (q % tiles_x))) * min(8, height - 8 * (q // tiles_x))
        for q, kd in enumerate(kinds) if base_kind(kd) == kind)
    wide_pixels = sum(min(8, width - 8 * (q % tiles_x)) for q in wide)
    foreign = in_target("F") + 3 * count("M")
    unsupported = int(np.isin(k, [q for q in range(n) if owner[q] >= 0 and base_kind(kinds[owner[q]]) == "X"])[vis != 0].sum())
    written = 64 * (count("O") + count("K")) + 22 * count("M") + in_target("Px", True) + in_target("Py") + 16 * count("SG") + wide_pixels
    keys = count("O") + 64 * count("K") + 3 * count("M") + in_target("Px", True) + count("Py") + count("S") + 3 * count("SG") + count("X") + (1 if wide else 0)
    covered = written + foreign + len(stale) + unsupported
    assert covered == int((vis != 0).sum()) and (unsupported > 0) == (count("X") > 0), name
    expect = dict(resolve=dict(covered_pixels=covered, visible_commands=n, foreign_pixels=foreign),
                  compact=dict(covered_pixels=covered, foreign_pixels=foreign, visible_commands=n, visible_triangles=keys,
                               written_commands=n, range_errors=0),
                  surface=dict(covered_pixels=covered, written_pixels=written, foreign_pixels=foreign, unsupported_pixels=unsupported,
                               stale_pixels=len(stale), degenerate_pixels=in_target("Py")))
    p = Programme(name, width, height, tuple(kinds), vis, pk, expect=expect)
    p.surface = sc.SurfaceCase(name, vis, pk, BASE, expect=expect["surface"], stale=stale)
    p.compact = cc.CompactCase(name, vis, pk.words, pk.max_commands, pk.meshlet_data, BASE, pk.meshlet_data_words,
                               expect=expect["compact"])
    return p


def parse(rows):
    return tuple(k for row in rows for k in row.split())


# 73 x 33: 10 x 5 tiles, column 9 one pixel wide, row 4 one pixel high.  Under a cap of 1 wave g takes g, g + 4, ..., under a
# cap of 2 g, g + 8, ...: K > O > K are tiles 6, 10, 14 and 2, 10, 18, the ring's r32 and r0 are tiles 15 and 31 — wave 3 of one workgroup,
# wave 7 of two —, its r33 tile 30.  The layout was found by a search over arrangements(); tests/test_visibility_tiles_cpu.py asserts what it holds
MAIN_W, MAIN_H = 73, 33
MAIN_KINDS = parse((
    "O     SG    K        S:entity E  X  K        O  E        Px",
    "O     E     O        O        K  O:r32  S:index  F  K    Px",
    "O     X     S:entity E        O  O  S:corner M  S:entity Px",
    "O:r33 O:r0  O        F        O  O  S:entity O  X        Px",
    "Py    Py    Py       Py       Py Py Py       Py Py       Py",
))


def programmes():
    """-> [Programme]: the 73 x 33 target; a 16 x 16 target of four tiles, each a wave's only tile under every cap; the
    7 x 5 target of one tile, three waves without one; a 65 x 8 target of one tile row whose tiles 0, 4 and 8 (the partial
    column) share the W key: wave 0 of one workgroup takes all three, wave 0 of two takes 0 and 8"""
    return [programme("tiles_73x33", MAIN_W, MAIN_H, MAIN_KINDS),
            programme("four_tiles_16x16", 16, 16, ("O", "F", "E", "K")),
            programme("one_tile_7x5", 7, 5, ("Px",)),
            programme("one_row_65x8", 65, 8, ("W", "O", "E", "K", "W", "F", "O", "M", "W"))]


def arrangements_of(progs, cap, resident=RESIDENT):
    return set().union(*(arrangements(p.kinds, p.tiles, cap, resident) for p in progs))


UNCAPPED = ("c:F_alone", "e:SG", "g:two_waves", "h:idle_wave")  # what is left when every wave takes one tile


# ------------------------------------------------------------------------------------------ the totals' second round
def sparse_buffer(keys, w=65, h=25):
    """A (h, w) buffer whose pixel p < len(keys) holds keys[p] = (command id, triangle); the rest is uncovered."""
    assert len(keys) <= w * h
    p = np.arange(len(keys), dtype=np.int64)
    keys = np.asarray(keys, np.int64).reshape(-1, 2)
    words = np.zeros(w * h, np.uint64)
    words[:len(keys)] = _word((F(0.25) + (p % 7).astype(F) / F(16)).astype(F), keys[:, 0], keys[:, 1])
    return words.reshape(h, w)


def long_list(n, shape_of):
    """visibility_compact_cases.build_list for lists of 10^5 commands: n commands, command k of shape_of(k) = (nt, vcount,
    misalign), all of them sharing the index words and corner bytes of the first four (no raster reads them).
    -> ({count; commands} words, meshlet_data)"""
    words4, data = cc.build_list([shape_of(k) for k in range(4)])
    assert all(shape_of(k) == shape_of(k % 4) for k in (4, 5, 6, 7, n - 1))
    cmds = np.tile(words4[1:].reshape(4, 7), ((n + 3) // 4, 1))[:n].copy()
    cmds[:, 4], cmds[:, 5], cmds[:, 6] = np.arange(n) % 7, 1000 + np.arange(n), 5000 + np.arange(n)
    words = np.zeros(1 + 7 * n, np.uint32)
    words[0], words[1:] = n, cmds.reshape(-1)
    return words, data


def second_round_cases():
    """-> [cc.CompactCase].  `expect` holds the counters; `claims` (added to each case) the (position j in the output,
    command id) pairs known in closed form: everything in front of j is the carry that reached it.
      chunks_258               257 * CHUNK + 5 commands, 258 blocks, two rounds of the totals.  Visible: commands 3, 77 and
                               CHUNK - 1 of chunk 0, nothing of chunks 1 to 254, all of chunk 255, three of chunk 256, all
                               five of chunk 257.  m = 1, 2, 3, 4 in turn and vcount 3: regions of 4, 5, 6, 6 words
      chunks_257_listed_short  max_commands 300 * CHUNK, 256 * CHUNK + 3 listed: the carry of block 256, the first of round
                               two, is the whole of round one; the blocks behind it do nothing
      chunks_512_exact         512 * CHUNK commands, two full rounds: the first and the last command of blocks 0 and 256"""
    out = []
    shape = lambda k: (8, 3, k % 4)  # noqa: E731
    m_of = lambda k: 1 + k % 4  # noqa: E731
    size_of = lambda k: 3 + (3 * m_of(k) + 3) // 4  # noqa: E731

    def add(name, n, visible, max_commands=None, claims=()):
        words, data = long_list(n, shape)
        keys = [(k, 2 * t) for k in visible for t in range(m_of(k))]
        case = cc.CompactCase(name, sparse_buffer(keys), words, n if max_commands is None else max_commands, data, 0,
                              expect=dict(visible_commands=len(visible), visible_triangles=len(keys), range_errors=0,
                                          written_commands=len(visible), dropped_commands=0, covered_pixels=len(keys), foreign_pixels=0),
                              expect_cut=dict(data_words_needed=sum(size_of(k) for k in visible)))
        if max_commands is not None:  # the words behind the listed commands: never read as commands
            case.words = np.concatenate([words, np.full(7 * (max_commands - n), 0xDEADBEEF, np.uint32)])
        case.claims = [(visible.index(k), k) for k in claims]
        out.append(case)

    n = 257 * CHUNK + 5
    visible = [3, 77, CHUNK - 1] + list(range(255 * CHUNK, 256 * CHUNK)) + [256 * CHUNK + q for q in (0, 100, 255)] + \
        list(range(257 * CHUNK, n))
    add("chunks_258", n, visible, claims=(256 * CHUNK, 257 * CHUNK, n - 1))
    n = 256 * CHUNK + 3
    visible = [0, CHUNK] + list(range(255 * CHUNK + 250, n))
    add("chunks_257_listed_short", n, visible, max_commands=300 * CHUNK, claims=(256 * CHUNK, n - 1))
    n = 512 * CHUNK
    visible = [b * CHUNK + q for b in (0, 256) for q in (0, CHUNK - 1)]
    add("chunks_512_exact", n, visible, claims=(256 * CHUNK, 257 * CHUNK - 1))
    return out


def second_round_capacities(stats):
    """Those of cc.capacity_variants that put the prefix cut into round two -> [(name, overrides, triangles)].
    `visible_capacity` exact and `visible_data_words` exact are ONE variant here, capacity_exact, which sets both to what
    the list needs; capacity_one_less and data_words_one_less lower one of the two by one.  The two plain_ variants, the
    same two capacities without ORBIT_COMPACT_TRIANGLES, are an addition."""
    keep = ("capacity_exact", "capacity_one_less", "data_words_one_less", "plain_capacity_exact", "plain_capacity_one_less")
    return [v for v in cc.capacity_variants(stats) if v[0] in keep]


# ------------------------------------------------------------------------------------------------ the resolve's clear
RESOLVE_CLEAR_COMMANDS = 5000  # five rounds of 1024 entries for one workgroup of resolve_clear_kernel


# ------------------------------------------------------------------------------------------------ the natural grid
def natural_target(num_cus, width=1921, height=1081):
    """-> (width, height, waves): 1921 x 1081, or taller until the resident grid of num_cus * 8 workgroups takes three
    trips over its tiles; a pixel wide and a pixel high in its last tiles either way"""
    waves = WAVES * 8 * num_cus
    tiles_x = (width + 7) // 8
    while tiles_x * ((height + 7) // 8) <= 2 * waves:
        height += 8 * ((2 * waves) // tiles_x + 1 - (height + 7) // 8) + 8
    assert width % 8 == 1 and height % 8 == 1
    return width, height, waves


def instanced(prog, width, height, waves):
    """prog's meshes (without the hand-written faults: the S commands are ordinary triangles here) four times, moved by
    entity translations of whole tiles: into the target's top right corner — the first trip, the partial column —, to the
    left of its middle row — a middle trip —, into its bottom left corner — the partial row —, and into its bottom right
    corner, the last tile of the last trip.  The three first are pushed 0.2 away and the last 0.2 nearer: what a Py
    triangle spills over the corner loses there, and none of the three lies to the right of and below another.
    -> (rc.Packed, [(name, offset x, offset y, trip of its first tile, trip of its last tile)])"""
    assert prog.width <= width // 4 and prog.height <= height // 4
    tiles_x = (width + 7) // 8
    mid_y = 8 * ((height // 8) // 2)
    places = (("top_right", width - prog.width, 0, -0.2), ("middle", 8 * ((width // 8) // 2 - prog.width // 8), mid_y, -0.2),
              ("bottom_left", 0, height - prog.height, -0.2), ("bottom_right", width - prog.width, height - prog.height, 0.2))
    entities, meshlets, where = [], [], []
    for i, (name, dx, dy, dz) in enumerate(places):
        assert dx % 8 == 0 and dy % 8 == 0
        move = np.eye(4, dtype=F)
        move[0, 3], move[1, 3], move[2, 3] = dx, dy, dz
        entities += [np.ascontiguousarray(move.T.reshape(16)), np.ascontiguousarray((move * F(2.0) ** F(-100)).T.reshape(16))]
        meshlets += [rc.Meshlet(m.positions, m.corners, 2 * i + m.entity) for m in prog.packed.case.meshlets]
        first = (dy // 8) * tiles_x + dx // 8
        last = ((dy + prog.height - 1) // 8) * tiles_x + (dx + prog.width - 1) // 8
        where.append((name, dx, dy, first // waves, last // waves))
    case = wk.WalkCase(f"{prog.name}_four_times", meshlets, width=width, height=height, entities=entities, command_base=BASE,
                       clip_near=True)
    return rc.Packed(case), where
