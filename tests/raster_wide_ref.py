"""An independent restatement of the raster calls WITH ORBIT_RASTER_WIDE_GUARD (include/orbit_abi_ext.h R4w, R5w-R7w over
R1-R9, R3c and V1-V4).  It shares no code with the library, with orbit_amd/csrc/raster_common.h or with the host mirror,
and it is a different walk from both: snapped coordinates, areas and edge functions are Python integers (exact at any
width), and coverage is not found by evaluating samples — per pixel row each edge's inside interval is SOLVED by exact
integer division and the three are intersected.  R2-R4 and R7 are np.float32 step by step, R7w is np.float64 step by
step.  Without the flag it restates the unflagged calls (a vertex outside R4's band is then out of band).  One walk
serves both calls: it builds the visibility words; the depth call's result is their high halves (V4).
tests/test_raster_wide_cpu.py holds the host mirror to it."""
import math

import numpy as np

F, D = np.float32, np.float64
STAT_NAMES = ("commands", "triangles", "clip_skipped", "guard_skipped", "back_facing", "no_coverage", "fragments",
              "range_errors")
CLEAR, CULL_NONE, CLIP_NEAR, WIDE_GUARD = 1, 2, 8, 32
PRIORITY = ("drawn", "guard_skipped", "back_facing", "no_coverage")  # a clipped triangle counts under its best piece
NARROW, WIDE, OUT = "narrow", "wide", "out"


def _mvp(a, b):
    out = np.zeros(16, F)
    for c in range(4):
        for r in range(4):
            acc = F(a[r] * b[4 * c])
            for k in (1, 2, 3):
                acc = F(acc + F(a[4 * k + r] * b[4 * c + k]))
            out[4 * c + r] = acc
    return out


def _clip(mvp, p):
    return tuple(F(F(F(F(mvp[r] * p[0]) + F(mvp[4 + r] * p[1])) + F(mvp[8 + r] * p[2])) + F(mvp[12 + r] * F(1)))
                 for r in range(4))


def _inside_r3(c):
    x, y, z, w = c
    return bool(w > 0 and z >= 0 and z <= w)


def snap(x, y, w, width, height, wide):
    """R4 / R4w -> (X, Y, NARROW | WIDE | OUT); X, Y are Python integers (0 when out of band)"""
    xf = F(F(F(F(F(x / w) * F(0.5)) + F(0.5)) * F(width)) * F(256))
    yf = F(F(F(F(F(y / w) * F(-0.5)) + F(0.5)) * F(height)) * F(256))
    if abs(xf) < F(2 ** 23) and abs(yf) < F(2 ** 23):
        return int(np.rint(xf)), int(np.rint(yf)), NARROW
    if wide and abs(xf) < F(2 ** 60) and abs(yf) < F(2 ** 60):  # (false for NaN)
        return int(np.rint(xf)), int(np.rint(yf)), WIDE  # a float of 2^23 or more is an integer: nothing is rounded
    return 0, 0, OUT


def _vertex(c, width, height, wide):
    X, Y, kind = snap(c[0], c[1], c[3], width, height, wide)
    return X, Y, F(c[2] / c[3]), kind


def _new_vertex(i, o, width, height, wide):
    """N(i, o) of R3c, or None: the whole triangle is clip_skipped"""
    b_i, b_o = F(i[3] - i[2]), F(o[3] - o[2])
    den = F(b_i - b_o)
    if not den > 0:
        return None
    t = F(b_i / den)
    x, y, w = (F(i[k] + F(t * F(o[k] - i[k]))) for k in (0, 1, 3))
    if not w > 0:
        return None
    X, Y, kind = snap(x, y, w, width, height, wide)
    return X, Y, F(1.0), kind


def pieces_of(c, width, height, wide, clip_near):
    """-> (pieces, form): a piece is three (X, Y, d, kind); form "whole", "skipped", "one_in" or "one_out"."""
    ins = [_inside_r3(v) for v in c]
    if all(ins):
        return [tuple(_vertex(v, width, height, wide) for v in c)], "whole"
    finite = all(math.isfinite(float(q)) for v in c for q in v)
    if not (clip_near and finite and all(v[2] >= 0 for v in c) and any(ins)):
        return [], "skipped"
    if sum(ins) == 1:
        k = ins.index(True)
        a, b, cc = c[k], c[(k + 1) % 3], c[(k + 2) % 3]
        nb, nc = _new_vertex(a, b, width, height, wide), _new_vertex(a, cc, width, height, wide)
        if nb is None or nc is None:
            return [], "skipped"
        return [(_vertex(a, width, height, wide), nb, nc)], "one_in"
    k = ins.index(False)
    a, b, cc = c[k], c[(k + 1) % 3], c[(k + 2) % 3]
    p, q = _new_vertex(b, a, width, height, wide), _new_vertex(cc, a, width, height, wide)
    if p is None or q is None:
        return [], "skipped"
    vb, vc = _vertex(b, width, height, wide), _vertex(cc, width, height, wide)
    return [(vb, vc, q), (vb, q, p)], "one_out"


def row_interval(tx, ty, y, x_lo, x_hi):
    """The pixels x of row y whose sample (256 x + 128, 256 y + 128) is inside the triangle (orientation A > 0), as one
    interval [lo, hi] (empty when lo > hi): each edge's condition is linear in x and solved by floor division."""
    py = 256 * y + 128
    lo, hi = x_lo, x_hi
    for u, v in ((0, 1), (1, 2), (2, 0)):
        dx, dy = tx[v] - tx[u], ty[v] - ty[u]
        top_left = dy < 0 or (dy == 0 and dx > 0)
        c = dx * (py - ty[u]) - (0 if top_left else 1)  # inside <=> c - dy * (px - tx[u]) >= 0
        if dy == 0:
            if c < 0:
                return 1, 0
        elif dy > 0:  # px <= tx[u] + floor(c / dy)
            hi = min(hi, (tx[u] + c // dy - 128) // 256)
        else:  # px >= tx[u] + ceil(c / dy) = tx[u] - floor(c / -dy)
            lo = max(lo, -((128 - (tx[u] - c // (-dy))) // 256))
    return lo, hi


def covered_samples(tx, ty, box):
    """-> (xs, ys) int64 arrays of the inside samples of the box, row by row"""
    x_lo, x_hi, y_lo, y_hi = box
    xs, ys = [], []
    for y in range(y_lo, y_hi + 1):
        lo, hi = row_interval(tx, ty, y, x_lo, x_hi)
        if lo <= hi:
            xs.append(np.arange(lo, hi + 1, dtype=np.int64))
            ys.append(np.full(hi - lo + 1, y, np.int64))
    if not xs:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(xs), np.concatenate(ys)


def wrapped_samples(tx, ty, box):
    """What an implementation whose edge products wrapped to 64 bits would cover: every sample of the box, in uint64
    arithmetic read as int64.  Only for the cases' own check that they need more than 64 bits."""
    x_lo, x_hi, y_lo, y_hi = box
    u64 = lambda v: np.uint64(v % 2 ** 64)  # noqa: E731
    px = (256 * np.arange(x_lo, x_hi + 1, dtype=np.int64) + 128).astype(np.uint64)[None, :]
    py = (256 * np.arange(y_lo, y_hi + 1, dtype=np.int64) + 128).astype(np.uint64)[:, None]
    inside = np.ones((y_hi - y_lo + 1, x_hi - x_lo + 1), bool)
    for u, v in ((0, 1), (1, 2), (2, 0)):
        dx, dy = tx[v] - tx[u], ty[v] - ty[u]
        nb = 0 if (dy < 0 or (dy == 0 and dx > 0)) else 1
        e = u64(dx) * (py - u64(ty[u])) - u64(dy) * (px - u64(tx[u])) - u64(nb)
        inside &= e.view(np.int64) >= 0
    yy, xx = np.nonzero(inside)
    return xx + x_lo, yy + y_lo


def oriented(piece, cull_none):
    """R5 / R5w in integers -> ("no_coverage" | "back_facing", None) or ("drawn", (tx, ty, td, area)) with A > 0"""
    (x0, y0, d0, _), (x1, y1, d1, _), (x2, y2, d2, _) = piece
    area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    if area == 0:
        return "no_coverage", None
    if area > 0 and not cull_none:
        return "back_facing", None
    if area < 0:
        x1, y1, d1, x2, y2, d2, area = x2, y2, d2, x1, y1, d1, -area
    return "drawn", ((x0, x1, x2), (y0, y1, y2), (d0, d1, d2), area)


def box_of(tx, ty, width, height):
    return (max(-((128 - min(tx)) // 256), 0), min((max(tx) - 128) // 256, width - 1),
            max(-((128 - min(ty)) // 256), 0), min((max(ty) - 128) // 256, height - 1))


def plane_depths(tx, ty, td, area, xs, ys, wide):
    """R7 (np.float32) or R7w (np.float64) at the samples -> np.float32, clamped to 1"""
    px, py = 256 * xs + 128, 256 * ys + 128
    if not wide:
        d10, d20, area_f = F(td[1] - td[0]), F(td[2] - td[0]), F(float(area))
        gx = F(F(F(d10 * F(ty[2] - ty[0])) - F(d20 * F(ty[1] - ty[0]))) / area_f)
        gy = F(F(F(d20 * F(tx[1] - tx[0])) - F(d10 * F(tx[2] - tx[0]))) / area_f)
        dd = (td[0] + gx * (px - tx[0]).astype(F)) + gy * (py - ty[0]).astype(F)
    else:
        hi, lo = area >> 64, area & (2 ** 64 - 1)
        area_d = D(D(float(hi)) * D(2.0 ** 64)) + D(float(lo))  # float(int) rounds to nearest even, as the conversions do
        d10, d20 = D(D(td[1]) - D(td[0])), D(D(td[2]) - D(td[0]))
        gx = D(D(D(d10 * D(float(ty[2] - ty[0]))) - D(d20 * D(float(ty[1] - ty[0])))) / area_d)
        gy = D(D(D(d20 * D(float(tx[1] - tx[0]))) - D(d10 * D(float(tx[2] - tx[0])))) / area_d)
        # (differences are below 2^62: int64 holds them, and int64 -> float64 rounds to nearest even)
        dd = (D(td[0]) + gx * (px - tx[0]).astype(D)) + gy * (py - ty[0]).astype(D)
        assert dd.dtype == D
        dd = dd.astype(F)
    assert dd.dtype == F
    return np.where(F(1) < dd, F(1), dd)


def exact_error(tx, ty, td, area, xs, ys, dd):
    """max over the samples of d - d_exact, in units of ulp(d) (a float; -inf without samples), where d_exact is the
    plane through the three fp32 vertex depths in exact rationals: all numerators over the common denominator
    A * 2^149, in Python integers."""
    m = [int(np.float64(t) * 2.0 ** 149) for t in td]  # fp32 values are multiples of 2^-149: exact
    m10, m20 = m[1] - m[0], m[2] - m[0]
    cx, cy = m10 * (ty[2] - ty[0]) - m20 * (ty[1] - ty[0]), m20 * (tx[1] - tx[0]) - m10 * (tx[2] - tx[0])
    worst = -math.inf
    for x, y, d in zip(xs.tolist(), ys.tolist(), dd.tolist()):
        num = m[0] * area + cx * (256 * x + 128 - tx[0]) + cy * (256 * y + 128 - ty[0])  # d_exact * A * 2^149
        if num > area << 149:  # clamped exactly as min(d, 1) clamps
            num = area << 149
        got = int(d * 2.0 ** 149)
        ulp = int(float(np.spacing(F(d))) * 2.0 ** 149)
        worst = max(worst, (got * area - num) / (area * ulp))
    return worst


def _draw_piece(piece, width, height, cull_none, vis, ident, extras, opts):
    kinds = [v[3] for v in piece]
    if OUT in kinds:
        extras["out_of_band_pieces"] += 1
        return "guard_skipped", 0
    wide = WIDE in kinds
    if wide:
        extras["wide_pieces"] += 1
        extras["max_coord_bits"] = max(extras["max_coord_bits"], max(abs(c) for v in piece for c in v[:2]).bit_length())
        # the same area in np.float64, every step rounded: where it calls a triangle degenerate and the integers do not
        (x0, y0, _, _), (x1, y1, _, _), (x2, y2, _, _) = piece
        a_d = D(D(D(float(x1 - x0)) * D(float(y2 - y0))) - D(D(float(x2 - x0)) * D(float(y1 - y0))))
        a_i = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
        extras["double_area_wrong"] += (a_d == 0) != (a_i == 0) or (a_d > 0) != (a_i > 0)
    verdict, tri = oriented(piece, cull_none)
    if tri is None:
        extras["wide_" + verdict] += wide
        return verdict, 0
    tx, ty, td, area = tri
    box = box_of(tx, ty, width, height)
    if box[0] > box[1] or box[2] > box[3]:
        extras["wide_off_target"] += wide
        return "no_coverage", 0
    if not wide:
        extras["lane_pieces" if (box[1] - box[0] + 1) * (box[3] - box[2] + 1) <= 16 else "wave_pieces"] += 1
    xs, ys = covered_samples(tx, ty, box)
    if wide:
        big = max(abs((tx[v] - tx[u]) * (256 * y + 128 - ty[u])) for u, v in ((0, 1), (1, 2), (2, 0)) for y in (box[2], box[3]))
        big = max(big, max(abs((ty[v] - ty[u]) * (256 * x + 128 - tx[u])) for u, v in ((0, 1), (1, 2), (2, 0)) for x in (box[0], box[1])))
        extras["beyond_64_bits"] += big >= 2 ** 63
        if opts.get("check_wrap") and big >= 2 ** 63:
            wx, wy = wrapped_samples(tx, ty, box)
            extras["wrap_differs"] += set(zip(wx.tolist(), wy.tolist())) != set(zip(xs.tolist(), ys.tolist()))
        extras["wide_small_box"] += (box[1] - box[0] + 1) * (box[3] - box[2] + 1) <= 16
    if len(xs) == 0:
        return "no_coverage", 0
    dd = plane_depths(tx, ty, td, area, xs, ys, wide)
    write = dd > 0
    if wide:
        extras["wide_drawn"] += 1
        extras["wide_samples"] += len(xs)
        if opts.get("exact"):
            extras["max_ulp_error"] = max(extras["max_ulp_error"], exact_error(tx, ty, td, area, xs[write], ys[write], dd[write]))
    word = (dd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(ident)
    vis[ys[write], xs[write]] = np.maximum(vis[ys[write], xs[write]], word[write])  # (the samples of a triangle are distinct)
    return "drawn", int(write.sum())


def new_extras():
    e = dict.fromkeys(("one_in", "one_out", "lane_pieces", "wave_pieces", "wide_pieces", "wide_drawn", "wide_samples",
                       "out_of_band_pieces", "wide_no_coverage", "wide_back_facing", "wide_off_target", "wide_small_box",
                       "beyond_64_bits", "wrap_differs", "double_area_wrong", "mixed_pieces", "max_coord_bits", "wide_triangles"), 0)
    e["max_ulp_error"] = -math.inf
    return e


def raster(words, max_commands, meshlet_data, vertices, vertex_count, entity_data, view_proj, width, height,
           visibility=None, command_base=0, flags=CLEAR | WIDE_GUARD, vertex_stride=12, position_offset=0, entity_count=None,
           meshlet_data_words=None, max_triangles=256, check_wrap=False, exact=False, draw_piece=None):
    """-> (visibility uint64 (height, width), stats dict, command_error list, extras dict).  max_triangles: V3's limit;
    None restates the depth call.  extras counts the routes: wide_pieces (pieces or whole triangles taken as wide),
    wide_triangles (triangles with one), mixed_pieces (two-piece triangles with one narrow and one wide piece),
    beyond_64_bits (wide pieces with an edge product of 2^63 or more on their box), wrap_differs (of those, with
    check_wrap: 64-bit wrapping changes the coverage), double_area_wrong (wide pieces whose area has another sign, or
    is zero, when evaluated in float64), max_ulp_error (with exact: see exact_error), and the rest.  draw_piece: a function to call in
    place of _draw_piece, for a tool that counts pieces instead of drawing them."""
    words = np.ascontiguousarray(words).view(np.uint8).reshape(-1).view(np.uint32)
    data = np.ascontiguousarray(meshlet_data, dtype=np.uint32).reshape(-1)
    data_words = len(data) if meshlet_data_words is None else meshlet_data_words
    corner_bytes = data.view(np.uint8)
    vb = np.ascontiguousarray(vertices).view(np.uint8).reshape(-1)
    ent = np.ascontiguousarray(entity_data).view(np.uint8).reshape(-1).view(F).reshape(-1, 32)
    entity_count = len(ent) if entity_count is None else entity_count
    vp = np.asarray(view_proj, F).reshape(16)
    vis = (np.zeros((height, width), np.uint64) if flags & CLEAR
           else np.array(visibility, np.uint64).reshape(height, width).copy())
    clip_near, cull_none, wide = bool(flags & CLIP_NEAR), bool(flags & CULL_NONE), bool(flags & WIDE_GUARD)
    st = dict.fromkeys(STAT_NAMES, 0)
    extras, opts = new_extras(), dict(check_wrap=check_wrap, exact=exact)
    draw_piece = draw_piece or _draw_piece
    errors = []
    old = np.seterr(all="ignore")
    try:
        for i in range(min(int(words[0]), max_commands)):
            index_count, _, first_index, index_base, entity, vertex_base, _ = (int(w) for w in words[1 + 7 * i:8 + 7 * i])
            nt, first_word = index_count // 3, first_index // 4
            vcount = first_word - index_base
            st["commands"] += 1
            bad = (first_word < index_base or vcount > 255 or first_word > data_words
                   or (max_triangles is not None and nt > max_triangles)
                   or (first_index + 3 * nt + 3) // 4 > data_words or entity >= entity_count)
            if not bad:
                gv = vertex_base + data[index_base:index_base + vcount].astype(np.int64)
                corners = corner_bytes[first_index:first_index + 3 * nt].reshape(nt, 3).astype(np.int64)
                bad = bool((gv >= vertex_count).any() or (corners >= vcount).any())
            errors.append(int(bad))
            if bad:
                st["range_errors"] += 1
                continue
            st["triangles"] += nt
            mvp = _mvp(vp, ent[entity][:16])
            clips = [_clip(mvp, vb[g * vertex_stride + position_offset:][:12].view(F)) for g in gv]
            for t, tri in enumerate(corners):
                pieces, form = pieces_of([clips[k] for k in tri], width, height, wide, clip_near)
                if not pieces:
                    st["clip_skipped"] += 1
                    continue
                if form != "whole":
                    extras[form] += 1
                before = extras["wide_pieces"]
                ident = (command_base + i) << 8 | (t & 255)
                results = [draw_piece(p, width, height, cull_none, vis, ident, extras, opts) for p in pieces]
                extras["wide_triangles"] += extras["wide_pieces"] > before
                extras["mixed_pieces"] += len(pieces) == 2 and extras["wide_pieces"] - before == 1 and all(r == "drawn" for r, _ in results)
                st["fragments"] += sum(n for _, n in results)
                best = min((r for r, _ in results), key=PRIORITY.index)
                if best != "drawn":
                    st[best] += 1
    finally:
        np.seterr(**old)
    return vis, st, errors, extras


def depth_of(visibility):
    """the high halves as floats: what the depth call leaves (V4)"""
    return (np.asarray(visibility, np.uint64) >> np.uint64(32)).astype(np.uint32).view(F)


def raster_depth(words, max_commands, meshlet_data, vertices, vertex_count, entity_data, view_proj, width, height,
                 depth=None, flags=CLEAR | WIDE_GUARD, **kw):
    """The depth call restated -> (depth float32 (height, width), stats, errors, extras)."""
    loaded = None if depth is None else np.asarray(depth, F).reshape(height, width).view(np.uint32).astype(np.uint64) << np.uint64(32)
    vis, st, errors, extras = raster(words, max_commands, meshlet_data, vertices, vertex_count, entity_data, view_proj,
                                     width, height, visibility=loaded, flags=flags, max_triangles=None, **kw)
    return depth_of(vis), st, errors, extras
