"""Inputs for orbit_visibility_surface_drawn (include/orbit_abi_ext.h S2d, S3c, S3w).  As in visibility_surface_cases, the
expected bytes are never computed here: the GPU tests' reference is the host mirror
(orbit_amd.raster.host_visibility_surface_drawn), which tests/test_surface_drawn_cpu.py holds to the restatement
tests/surface_drawn_ref.py; what a case CLAIMS (`expect`: counters known in closed form) is checked there.  Every buffer
comes from the host mirror's raster with the case's flags (raster_clip_cases.host_vis, raster_wide_cases.host_vis) and is
then, where the case says so, tampered with by hand.  A case's name ends in the flags it is READ with: @0, @8 (CLIP),
@32 (WIDE), @40.

Census:
  every case of visibility_surface_cases.all_cases()   read @0; and @40 where the buffer holds no cut or wide triangle
                                                        (everything but its clip_* cases): the same bytes as @0
  every case of raster_clip_cases.all_cases()           drawn with CLIP_NEAR, read @8: unsupported = 0, except
                                                        guard_piece_*, whose piece leaves the guard band (no claim @8);
                                                        those also drawn with both flags and read @40: unsupported = 0
  every case of raster_wide_cases.all_cases()           drawn and read with the flags the case uses (@32 or @40)
Hand cases on 7 x 5 and 65 x 9 (partial tiles on both edges), under raster_cases.w_from_z_proj unless said:
  one_in_full / one_out_full        a one-in and a one-out cut filling the target: every pixel is a cut pixel; the one-out
                                    cut's two pieces and their diagonal cross every tile
  *_mirror                          the same two mirror-wound, drawn with CULL_NONE: the piece's swap
  cut_with_a_wide_piece             one-out, piece (b, c, Q) narrow and piece (b, Q, P) wide (drawn with both flags)
  edge_ab_on_centres                exact_proj, t = 1/2: the original edge corner 0 - corner 2 of a one-in cut lies on the
                                    centres of the middle row: l1 (corner 1) is exactly 0 there
  diagonal_on_centres               exact_proj, one-out: the diagonal b-Q lies on the centres of the middle row, which
                                    exactly one piece owns
  cut_w_unequal                     a one-out cut with w = 0.05, 0.2, 0.8: l differs visibly from the screen-space value
65 x 9 only (an 8 x 8 tile of single-pixel keys at x = 8..15, y = 0..7; a cut key's piece is the pixel's triangle, a
wide key is a sliver from the pixel to a vertex 2^24 sub-pixels to the left, behind everything else):
  64_keys_cut_and_wide              every second key a cut triangle, every eighth a wide one
  one_slow_of_64 / one_fast_of_64   exactly one slow key beside 63 fast ones, and the reverse
  cut_t_255_of_256                  nt = 256: triangle 255 is the cut one
Stale and unsupported, each with one tampered pixel (`stale` / `unsupported`: the tampered pixels):
  stale_depth_bit_in_piece_1        one bit of a high half flipped at a pixel of piece 1 of one_out_full_65x9
  stale_moved_outside_both_pieces   a word of raster_clip_cases' lone_out_vertex_0 copied to a pixel outside both pieces
  unsupported_cut_key_without_clip  a word naming a cut triangle, in a buffer drawn and read without CLIP (@0, @32):
                                    unsupported, status OK
  stale_out_of_band_key             a word naming raster_wide_cases' band_top_2_60_is_out, read @32: stale"""
from dataclasses import dataclass, field

import numpy as np

import raster_cases as rc
import raster_clip_cases as clip
import raster_wide_cases as wide
import visibility_surface_cases as sc
from raster_cases import poly, w_from_z_proj
from raster_clip_cases import exact_proj
from raster_vis_cases import _word
from raster_wide_cases import WideCase

F = np.float32
CLIP, WIDE = 8, 32
BOTH = CLIP | WIDE
HAND_SIZES = ((7, 5), (65, 9))
IN, OUT = 0.2, 0.05


@dataclass
class DrawnCase(sc.SurfaceCase):
    raster_flags: int = 0
    unsupported: list = field(default_factory=list)  # (y, x) tampered with, expected unsupported
    zero_l1_row: int = None     # every written pixel of this row has l1 == +0.0f exactly
    both_pieces: bool = False   # pixels of both pieces are written
    same_as: str = None         # the case @0 whose bytes this one must give

    def args(self, **over):
        a, kw = super().args(**over)
        kw.setdefault("raster_flags", self.raster_flags)
        return a, kw


def read(name, vis, pk, base, flags, **kw):
    return DrawnCase(f"{name}@{flags}", vis, pk, base, raster_flags=flags, **kw)


def drawn(case, flags, **kw):
    """A WideCase -> DrawnCase over the buffer the host mirror's raster gives it with the case's flags, read with `flags`"""
    pk = rc.Packed(case)
    vis = wide.host_vis(pk, wide=bool(flags & WIDE), clip_near=bool(flags & CLIP))[0]
    return read(case.name, vis, pk, getattr(case, "command_base", 0), flags, **kw)


# -------------------------------------------------------------------------------------------------- the census
def inherited_cases():
    out = []
    for c in sc.all_cases():
        common = dict(words=c.words, max_commands=c.max_commands, expect=dict(c.expect), stale=list(c.stale))
        zero = read(c.name, c.visibility, c.packed, c.command_base, 0, **common)
        zero.clean = None if c.clean is None else read(c.clean.name, c.clean.visibility, c.clean.packed, c.clean.command_base, 0)
        out.append(zero)
        if not c.name.startswith("clip_"):
            both = read(c.name, c.visibility, c.packed, c.command_base, BOTH, same_as=zero.name, **common)
            both.clean = None if c.clean is None else read(c.clean.name, c.clean.visibility, c.clean.packed, c.clean.command_base, BOTH)
            out.append(both)
    return out


def clip_cases():
    out = []
    for c in clip.all_cases():
        pk = rc.Packed(c)
        base = getattr(c, "command_base", 0)
        leaves_band = c.name.startswith("guard_piece_")
        expect = dict(stale_pixels=0) if leaves_band else dict(stale_pixels=0, unsupported_pixels=0)
        out.append(read("clip_" + c.name, clip.host_vis(pk)[0], pk, base, CLIP, expect=expect))
        if leaves_band:
            vis = wide.host_vis(pk, wide=True, clip_near=True)[0]
            out.append(read("clip_" + c.name, vis, pk, base, BOTH, expect=dict(stale_pixels=0, unsupported_pixels=0)))
    return out


def wide_cases():
    return [drawn(c, WIDE | (CLIP if c.clip_near else 0), expect=dict(stale_pixels=0, unsupported_pixels=0)) for c in wide.all_cases()]


# -------------------------------------------------------------------------------------------------- hand-built
def ndc(x, y, w):
    """the model position under w_from_z_proj (or exact_proj) at ndc (x, y) (y up) and clip w"""
    return (x * w, y * w, w)


def on_screen(sx, sy, w, width, height):
    """the same from framebuffer coordinates (y down)"""
    return ndc(2.0 * sx / width - 1.0, 1.0 - 2.0 * sy / height, w)


def case(name, w, h, tris, **kw):
    kw.setdefault("view_proj", w_from_z_proj())
    return WideCase(f"{name}_{w}x{h}", [poly(t) if isinstance(t, list) else poly([t]) for t in tris], width=w, height=h, **kw)


ONE_IN = (ndc(-1.5, -1.5, IN), ndc(18.0, -1.5, OUT), ndc(-1.5, 18.0, OUT))   # its piece (fractions 1/3) covers the target
# the quad (b, c, Q, P) = (-3, -3), (3, -3), (2, 3), (-2, 3) covers the target; both its diagonals pass by the centre (the mirror's is c-P)
ONE_OUT = (ndc(0.0, 15.0, OUT), ndc(-3.0, -3.0, IN), ndc(3.0, -3.0, IN))
# exact_proj (near 0.125), out vertices at w = 0, in vertices at w = 0.25: t = 1/2, new vertices at w = 0.125, ndc y = 0 is
# the centre of the middle row of a target of odd height
EDGE_ON_CENTRES = ((-0.2, 0.0, 0.25), (-0.2, -0.225, 0.0), (0.4, 0.0, 0.0))     # (a, c, b): l1 is corner c's
DIAGONAL_ON_CENTRES = ((0.0, 0.2, 0.0), (-0.2, 0.0, 0.25), (0.2, -0.2, 0.25))   # (a out, b, c)


def mirror(t):
    return (t[0], t[2], t[1])


def pixel_triangle(x, y, w, width, height):
    return tuple(on_screen(sx, sy, w, width, height) for sx, sy in ((x + 0.25, y + 0.25), (x + 0.25, y + 0.95), (x + 0.95, y + 0.25)))


def cut_pixel_triangle(x, y, width, height):
    """a one-in cut whose piece (a, N(a, b), N(a, c)) is pixel_triangle(x, y): the new vertices lie a third of the way to
    the out vertices on the screen (t = 2/3, w: 0.2 -> 0.1 -> 0.05)"""
    a, nb, nc = (x + 0.25, y + 0.25), (x + 0.25, y + 0.95), (x + 0.95, y + 0.25)
    far = lambda n: (a[0] + 3.0 * (n[0] - a[0]), a[1] + 3.0 * (n[1] - a[1]))  # noqa: E731
    return (on_screen(*a, IN, width, height), on_screen(*far(nb), OUT, width, height), on_screen(*far(nc), OUT, width, height))


def key_tile(name, kind):
    """an 8 x 8 tile of single-pixel keys at x = 8..15 of a 65 x 9 target; kind(q) -> "fast", "cut" or "wide" """
    w, h, tris = 65, 9, []
    for q in range(64):
        x, y = 8 + q % 8, q // 8
        tris.append({"fast": lambda: pixel_triangle(x, y, IN, w, h), "cut": lambda: cut_pixel_triangle(x, y, w, h),
                     "wide": lambda: wide_sliver(x, y, w, h)}[kind(q)]())
    return case(name, w, h, tris, clip_near=True, cull_none=True)


def wide_sliver(x, y, width, height):
    """a wide triangle through the sample of pixel (x, y) with its far vertex 2^24 sub-pixels to the left; w = 0.4: behind
    every pixel_triangle (w = 0.2) and every cut one"""
    return (on_screen(x + 0.95, y + 0.25, 0.4, width, height), on_screen(x + 0.95, y + 0.95, 0.4, width, height),
            on_screen(x - 65536.0, y + 0.55, 0.4, width, height))


def hand_cases():
    out = []
    full = lambda w, h: dict(covered_pixels=w * h, written_pixels=w * h, cut_pixels=w * h, unsupported_pixels=0, stale_pixels=0)  # noqa: E731
    for w, h in HAND_SIZES:
        out.append(drawn(case("one_in_full", w, h, [ONE_IN], clip_near=True), CLIP, expect=dict(full(w, h), wide_pixels=0)))
        out.append(drawn(case("one_out_full", w, h, [ONE_OUT], clip_near=True), CLIP, expect=dict(full(w, h), wide_pixels=0), both_pieces=True))
        out.append(drawn(case("one_in_full_mirror", w, h, [mirror(ONE_IN)], clip_near=True, cull_none=True), CLIP, expect=full(w, h)))
        out.append(drawn(case("one_out_full_mirror", w, h, [mirror(ONE_OUT)], clip_near=True, cull_none=True), CLIP, expect=full(w, h),
                         both_pieces=True))
        # the out vertex a far to the right; b = ndc (-0.9, -0.9) at w = 0.2 gives P = N(b, a) at t = 2/3, ndc x about 2000 (20000
        # on the narrow target, where 2^23 sub-pixels are ten times as many ndc units): wide.  c = ndc (-0.9, 0.9) a hair behind the
        # near plane gives Q = N(c, a) at t = 4e-4 (4e-5), ndc x = 0.3: narrow.  Piece (b, c, Q) is the upper left of the target and
        # narrow, piece (b, Q, P) the rest of it and wide.
        far, hair = (300.0, 2e-5) if w == 65 else (3000.0, 2e-6)
        out.append(drawn(case("cut_with_a_wide_piece", w, h, [((far, 0.0, OUT), (-0.18, -0.18, IN), (-0.09, 0.09, 0.1 + hair))], clip_near=True,
                              cull_none=True), BOTH, expect=dict(unsupported_pixels=0, stale_pixels=0), both_pieces=True))
        out.append(drawn(case("edge_ab_on_centres", w, h, [EDGE_ON_CENTRES], clip_near=True, view_proj=exact_proj()), CLIP,
                         expect=dict(unsupported_pixels=0, stale_pixels=0), zero_l1_row=h // 2))
        out.append(drawn(case("diagonal_on_centres", w, h, [DIAGONAL_ON_CENTRES], clip_near=True, view_proj=exact_proj()), CLIP,
                         expect=dict(unsupported_pixels=0, stale_pixels=0), both_pieces=True))
        out.append(drawn(case("cut_w_unequal", w, h, [(ndc(0.0, 19.0, OUT), ndc(-3.0, -2.0, IN), ndc(6.0, -2.0, 0.8))], clip_near=True), CLIP,
                         expect=full(w, h)))
    kinds = lambda q: "wide" if q % 8 == 0 else "cut" if q % 2 else "fast"  # noqa: E731
    tile = dict(unsupported_pixels=0, stale_pixels=0)
    out.append(drawn(key_tile("64_keys_cut_and_wide", kinds), BOTH, expect=dict(tile, cut_pixels=32)))
    out.append(drawn(key_tile("one_slow_of_64", lambda q: "cut" if q == 27 else "fast"), BOTH,
                     expect=dict(tile, covered_pixels=64, written_pixels=64, cut_pixels=1, wide_pixels=0)))
    out.append(drawn(key_tile("one_fast_of_64", lambda q: "fast" if q == 27 else "cut"), BOTH,
                     expect=dict(tile, covered_pixels=64, written_pixels=64, cut_pixels=63, wide_pixels=0)))
    flat = ((0.0, 0.0, 0.5),) * 3  # no area
    m = poly([flat] * 255 + [ONE_OUT])
    assert len(m.corners) == 256 and len(m.positions) == 4
    last = WideCase("cut_t_255_of_256_65x9", [m], width=65, height=9, view_proj=w_from_z_proj(), clip_near=True)
    out.append(drawn(last, CLIP, expect=dict(covered_pixels=65 * 9, written_pixels=65 * 9, cut_pixels=65 * 9, stale_pixels=0)))
    return out


def stale_cases():
    out = []

    def tampered(name, clean, edits, flags=None, unsupported=False):
        vis = clean.visibility.copy()
        for (y, x), word in edits:
            assert vis[y, x] != word
            vis[y, x] = word
        flags = clean.raster_flags if flags is None else flags
        where = [p for p, _ in edits]
        kw = dict(unsupported=where, expect=dict(unsupported_pixels=len(edits), stale_pixels=0)) if unsupported else \
            dict(stale=where, expect=dict(stale_pixels=len(edits)))
        c = read(name, vis, clean.packed, clean.command_base, flags, clean=clean, **kw)
        out.append(c)

    clean = drawn(case("one_out_full", 65, 9, [ONE_OUT], clip_near=True), CLIP)
    clean.name = "stale_clean_one_out@8"
    v = clean.visibility
    tampered("stale_depth_bit_in_piece_1", clean, [((0, 0), v[0, 0] ^ np.uint64(1 << 32))])  # top left: above the diagonal b-Q
    lone = next(c for c in clip.all_cases() if c.name == "lone_out_vertex_0")
    pk = rc.Packed(lone)
    clean = read("stale_clean_lone_out", clip.host_vis(pk)[0], pk, 0, CLIP)
    v = clean.visibility
    ys, xs = np.nonzero(v)
    assert v[0, 0] == 0
    tampered("stale_moved_outside_both_pieces", clean, [((0, 0), v[ys[0], xs[0]])])
    # an ordinary triangle (command 0) and a cut one (command 1) drawn WITHOUT the flag: the cut one owns nothing
    pair = case("plain_and_cut", 65, 9, [pixel_triangle(3, 3, IN, 65, 9), ONE_OUT])
    for flags in (0, WIDE):
        clean = drawn(pair, flags & WIDE)
        clean.name = f"unsupported_clean@{flags}"
        assert clean.visibility[7, 60] == 0 and int((clean.visibility != 0).sum()) == 1
        tampered("unsupported_cut_key_without_clip", clean, [((7, 60), _word(F(0.5), 1, 0))], flags=flags, unsupported=True)
    band = next(c for c in wide.all_cases() if c.name == "band_top_2_60_is_out")
    clean = drawn(band, WIDE)
    clean.name = "stale_clean_out_of_band@32"
    assert not clean.visibility.any()
    tampered("stale_out_of_band_key", clean, [((20, 20), _word(F(0.5), 0, 0))])
    return out


def all_cases():
    return inherited_cases() + clip_cases() + wide_cases() + hand_cases() + stale_cases()


def device_cases():
    """the clip, wide and hand cases: untampered buffers, which a device can draw itself with the case's flags"""
    return clip_cases() + wide_cases() + hand_cases()
