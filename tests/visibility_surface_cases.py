"""Inputs for orbit_visibility_surface (include/orbit_abi_ext.h S1-S7).  As in raster_cases, the expected bytes are never
computed here: the GPU tests' reference is the host mirror (orbit_amd.raster.host_visibility_surface), which
tests/test_visibility_surface_cpu.py holds to the numpy restatement tests/visibility_surface_ref.py; what a case CLAIMS
(`expect`: counters known in closed form) is checked against the restatement there.  A buffer comes from
host_raster_visibility of the case's own list (hand cases: 1 x 1, 7 x 5, 64 x 1, 65 x 9; the census keeps its own sizes)
and is then, where the case says so, tampered with by hand.

Census — rasterised, untouched (everything covered is written: stale = unsupported = 0):
  every case of raster_vis_cases.all_cases()   ties, nt = 256, the 257-triangle and the R9 commands the raster skipped
                                               (they own nothing), back faces drawn with CULL_NONE (the swap), count 0 and
                                               count > max_commands, command_base at the top of the 24 bits
  two_lists_base_0 / _base_cap                 both lists in one buffer, one call per base: the other list is foreign
General, hand-built:
  full_WxH               one triangle over 1 x 1, 7 x 5, 64 x 1, 65 x 9: partial 8 x 8 tiles on both edges, one key per tile
  64_keys_in_a_tile      one single-pixel triangle per pixel of an 8 x 8 block, 64 commands: 64 trips of the numbering loop
  t_0_63_64_255          nt = 256, 12 vertices: triangles 0, 63, 64, 255 own a pixel each, the others have no area
  list_65 / list_257     a pixel per command: more keys than lanes over the buffer, never in one tile
Swap:
  wound_front / wound_mirror   one triangle, and its mirror-wound copy drawn with CULL_NONE: the same l per corner
Exact values (pixel_proj):
  vertex_on_centre_0/1/2 the triangle's top-left vertex on a pixel centre, as corner 0, 1, 2: (0,0), (1,0), (0,1) exactly
  shared_edge            (the census' own) a diagonal through sample centres: the opposite corner's l is exactly 0
Perspective (w_from_z_proj):
  w_1_1_4                corners with w = 1, 1, 4: the pair differs from E / A and matches the rational value
Degenerate:
  w_2_pow_minus_120      all w = 2^-120: 1 / w times an edge value overflows, everything written is 0 and counted; no
                         denormal anywhere
  foreshortened          w = 1000, 1000, 0.1: just inside the far edge the +x neighbour has s <= 0: grad's x axis is zeroed
Foreign and edges of the list:
  range_ends             ids base - 1 and base + n (written by hand) beside base and base + n - 1 (drawn)
  ids_in_n_to_max        count 3 of max_commands 6, drawn with all 6: ids 3..5 are foreign (the resolve would own them)
  list_count_zero / list_count_above_max / base_top_of_24_bits
Stale, each alone in its buffer (`stale`: the tampered pixels; everything else as in the untouched run):
  stale_depth_bit        one bit of a high half flipped
  stale_moved_word       a word copied to the pixel beside its triangle
  stale_t_is_nt          t = nt
  stale_257_triangles    a word naming the 257-triangle command the raster skipped
  stale_r9_*             a word naming a command that fails R9: a corner byte, an index word, the entity, the ranges
Unsupported:
  every case of raster_clip_cases.all_cases() drawn with ORBIT_RASTER_CLIP_NEAR: pixels of cut triangles (unsupported)
  beside ordinary ones (written); status OK"""
from dataclasses import dataclass, field

import numpy as np

import raster_cases as rc
import raster_clip_cases as clip
import raster_vis_cases as vc
from raster_cases import Case, poly, tri
from raster_vis_cases import _word

F = np.float32
HAND_SIZES = ((1, 1), (7, 5), (64, 1), (65, 9))


@dataclass
class SurfaceCase:
    name: str
    visibility: np.ndarray   # (h, w) uint64
    packed: object           # rc.Packed: the list and its buffers
    command_base: int = 0
    words: np.ndarray = None        # overrides packed.words (another count)
    max_commands: int = None        # overrides packed.max_commands
    expect: dict = field(default_factory=dict)  # claimed counters
    stale: list = field(default_factory=list)   # (y, x) tampered with
    clean: object = None            # the untampered SurfaceCase of a stale one

    def args(self, **over):
        """-> (args, kwargs) of orbit_amd.raster.host_visibility_surface and visibility_surface_ref.surface"""
        kw, (words, mc, data, vb, vcount, ent, vp, w, h) = self.packed.args()
        kw = dict(kw, command_base=self.command_base)
        kw.update(over)
        return (self.visibility, words if self.words is None else self.words, mc if self.max_commands is None else self.max_commands,
                data, vb, vcount, ent, vp), kw


def drawn(case, **kw):
    """A raster_cases Case / VisCase -> SurfaceCase over the buffer the host mirror's raster gives it."""
    pk = rc.Packed(case)
    return SurfaceCase(case.name, vc.host(pk)[0], pk, getattr(case, "command_base", 0), **kw)


# -------------------------------------------------------------------------------------------------- rasterised
def rasterised_cases():
    out = [drawn(c, expect=dict(stale_pixels=0, unsupported_pixels=0, foreign_pixels=0)) for c in vc.all_cases()]
    a, b, cap = vc.two_lists()
    pa, pb = rc.Packed(a), rc.Packed(b)
    both = vc.host(pb, visibility=vc.host(pa)[0], clear=False)[0]
    out.append(SurfaceCase("two_lists_base_0", both, pa, 0, expect=dict(stale_pixels=0, unsupported_pixels=0)))
    out.append(SurfaceCase("two_lists_base_cap", both, pb, cap, expect=dict(stale_pixels=0, unsupported_pixels=0)))
    return out


def clip_cases():
    out = []
    for c in clip.all_cases():
        pk = rc.Packed(c)
        out.append(SurfaceCase("clip_" + c.name, clip.host_vis(pk)[0], pk, getattr(c, "command_base", 0), expect=dict(stale_pixels=0)))
    return out


# -------------------------------------------------------------------------------------------------- hand-built
def pixel_triangle(x, y, z=0.5):
    """A front-facing triangle that holds the one sample (x + 0.5, y + 0.5)."""
    return ((x + 0.25, y + 0.25, z), (x + 0.25, y + 0.95, z), (x + 0.95, y + 0.25, z))


def half_proj():
    """clip = (x, y, z / 2, z): the model's z is w, the depth is 1 / 2 everywhere, every product exact"""
    m = np.zeros(16, F)
    m[0], m[5], m[10], m[11] = 1, 1, F(0.5), 1
    return m


def general_cases():
    out = []
    for w, h in HAND_SIZES:
        out.append(drawn(Case(f"full_{w}x{h}", [tri((-1, -1), (-1, 3 * h + 2), (3 * w + 2, -1), z=0.75)], width=w, height=h),
                         expect=dict(covered_pixels=w * h, written_pixels=w * h, degenerate_pixels=0)))
    block = [poly([pixel_triangle(8 + q % 8, q // 8)]) for q in range(64)]
    out.append(drawn(Case("64_keys_in_a_tile", block, width=65, height=9), expect=dict(covered_pixels=64, written_pixels=64)))
    flat = ((0.0, 0.0, 0.5),) * 3  # no area
    tris = [flat] * 256
    for q, t in enumerate((0, 63, 64, 255)):
        tris[t] = pixel_triangle(3 + 9 * q, 2 + q)
    m = poly(tris)
    assert len(m.positions) == 13 and len(m.corners) == 256
    out.append(drawn(Case("t_0_63_64_255", [m], width=65, height=9), expect=dict(covered_pixels=4, written_pixels=4)))
    for n in (65, 257):
        out.append(drawn(Case(f"list_{n}", [poly([pixel_triangle(q % 65, q // 65)]) for q in range(n)], width=65, height=9),
                         expect=dict(covered_pixels=n, written_pixels=n)))
    return out


WOUND = ((3.3, 1.2), (9.1, 7.7), (40.6, 2.4))  # front-facing


def swap_cases():
    """-> (front, mirror): the mirror's corners 1 and 2 are the front's corners 2 and 1"""
    front = drawn(Case("wound_front", [poly([WOUND])], width=65, height=9), expect=dict(stale_pixels=0))
    mirror = drawn(Case("wound_mirror", [poly([(WOUND[0], WOUND[2], WOUND[1])])], width=65, height=9, cull_none=True),
                   expect=dict(stale_pixels=0))
    return front, mirror


ON_CENTRE = ((2.5, 1.5), (2.5, 6.5), (7.5, 1.5))  # its first vertex is the top-left one, on the centre of pixel (2, 1)


def exact_cases():
    out = []
    for k in range(3):  # the vertex on the centre as corner k
        corners = tuple(ON_CENTRE[(q - k) % 3] for q in range(3))
        out.append(drawn(Case(f"vertex_on_centre_{k}", [poly([corners])], width=65, height=9), expect=dict(stale_pixels=0)))
    return out


def perspective_case():
    corners = ((-0.5, -0.5, 1.0), (0.5, -0.5, 1.0), (-2.0, 2.0, 4.0))  # ndc (-0.5, -0.5), (0.5, -0.5), (-0.5, 0.5)
    return drawn(Case("w_1_1_4", [poly([corners])], width=65, height=9, view_proj=rc.w_from_z_proj()),
                 expect=dict(stale_pixels=0, degenerate_pixels=0))


def degenerate_cases():
    w = F(2.0) ** F(-120)
    tiny = tuple((F(x) * w, F(y) * w, w) for x, y in ((-0.5, -0.5), (0.5, -0.5), (-0.5, 0.5)))
    a = drawn(Case("w_2_pow_minus_120", [poly([tiny])], width=65, height=9, view_proj=half_proj()), expect=dict(stale_pixels=0))
    # the edge v0 -> v1 runs down the right side at ndc x = 0.5; v2, far to the left, is the near one
    far, near = 1000.0, 0.1
    fore = ((0.5 * far, -0.9 * far, far), (0.5 * far, 0.9 * far, far), (-0.9 * near, 0.0, near))
    b = drawn(Case("foreshortened", [poly([fore])], width=65, height=9, view_proj=rc.w_from_z_proj()), expect=dict(stale_pixels=0))
    return [a, b]


def five():
    return Case("five", [poly([pixel_triangle(2 + 3 * q, 1 + q)]) for q in range(5)], width=65, height=9)


def foreign_cases():
    out = []
    base, n = 1000, 5
    c = vc.VisCase(**{k: getattr(five(), k) for k in Case.__dataclass_fields__}, command_base=base)
    s = drawn(c)
    s.name = "range_ends"
    s.visibility[8, 60], s.visibility[8, 61] = _word(F(0.5), base - 1, 0), _word(F(0.5), base + n, 0)
    s.expect = dict(covered_pixels=7, written_pixels=5, foreign_pixels=2)
    out.append(s)
    six = Case("six", [poly([pixel_triangle(2 + 3 * q, 1 + q)]) for q in range(6)], width=65, height=9)
    s = drawn(six)
    s.name, s.words = "ids_in_n_to_max", s.packed.words.copy()
    s.words[0] = 3
    s.expect = dict(covered_pixels=6, written_pixels=3, foreign_pixels=3)
    out.append(s)
    s = drawn(five())
    s.name, s.words = "list_count_zero", s.packed.words.copy()
    s.words[0] = 0
    s.expect = dict(covered_pixels=5, written_pixels=0, foreign_pixels=5)
    out.append(s)
    s = drawn(five())
    s.name, s.words, s.max_commands = "list_count_above_max", s.packed.words.copy(), 3
    s.words[0] = 1000
    s.expect = dict(covered_pixels=5, written_pixels=3, foreign_pixels=2)
    out.append(s)
    top = (1 << 24) - 5
    c = vc.VisCase(**{k: getattr(five(), k) for k in Case.__dataclass_fields__}, command_base=top)
    s = drawn(c)
    s.name = "base_top_of_24_bits"
    s.visibility[8, 60] = _word(F(0.5), top - 1, 0)
    s.expect = dict(covered_pixels=6, written_pixels=5, foreign_pixels=1)
    out.append(s)
    return out


STALE_TRI = ((4.0, 1.0), (4.0, 8.0), (11.0, 1.0))  # covers the samples (4 + i, 1 + j), i + j <= 5


def stale_cases():
    out = []

    def tampered(name, clean, edits):
        vis = clean.visibility.copy()
        for (y, x), word in edits:
            assert vis[y, x] != word
            vis[y, x] = word
        out.append(SurfaceCase(name, vis, clean.packed, clean.command_base, stale=[p for p, _ in edits], clean=clean,
                               expect=dict(stale_pixels=len(edits))))

    clean = drawn(Case("stale_clean", [poly([STALE_TRI])], width=65, height=9), expect=dict(written_pixels=21, stale_pixels=0))
    v = clean.visibility
    assert v[2, 5] != 0 and v[2, 3] == 0 and v[1, 4] != 0
    tampered("stale_depth_bit", clean, [((2, 5), v[2, 5] ^ np.uint64(1 << 32))])
    tampered("stale_moved_word", clean, [((2, 3), v[2, 4])])
    tampered("stale_t_is_nt", clean, [((1, 4), v[1, 4] | np.uint64(1))])
    skipped = drawn(next(c for c in vc.new_cases() if c.name == "nt_257_between_neighbours"))
    assert skipped.visibility[40, 40] == 0
    tampered("stale_257_triangles", skipped, [((40, 40), _word(F(0.5), 1, 0))])
    for name in ("r9_corner_is_vcount", "r9_vertex_is_vertex_count", "r9_entity_is_entity_count", "r9_corner_bytes_beyond_data",
                 "r9_first_index_below_offset"):
        bad = drawn(next(c for c in vc.census_as_vis_cases() if c.name == name))
        assert bad.visibility[40, 40] == 0
        tampered("stale_" + name, bad, [((40, 40), _word(F(0.5), 1, 0))])
    return out


def hand_cases():
    front, mirror = swap_cases()
    return general_cases() + [front, mirror] + exact_cases() + [perspective_case()] + degenerate_cases() + foreign_cases()


def all_cases():
    return rasterised_cases() + hand_cases() + stale_cases() + clip_cases()
