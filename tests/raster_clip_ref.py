"""An independent numpy restatement of the raster calls WITH ORBIT_RASTER_CLIP_NEAR (include/orbit_abi_ext.h R3c over
R1-R9 and V1-V4): np.float32 arithmetic step by step, every operation rounded on its own, int64 edge functions at every
sample of a piece's box.  It keeps its own rotation and piece building, works triangle by triangle on scalars, and
shares no code with the library, with orbit_amd/csrc/raster_common.h or with the host mirror:
tests/test_raster_clip_cpu.py holds the mirror to it.  One walk serves both calls: it builds the visibility words, and
the depth call's result is their high halves (V4) with no limit on a command's triangles."""
import math

import numpy as np

F = np.float32
STAT_NAMES = ("commands", "triangles", "clip_skipped", "guard_skipped", "back_facing", "no_coverage", "fragments",
              "range_errors")
CLEAR, CULL_NONE, CLIP_NEAR = 1, 2, 8
PRIORITY = ("drawn", "guard_skipped", "back_facing", "no_coverage")  # a clipped triangle counts under its best piece


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
    """R2: clip = mvp x (p, 1)"""
    return tuple(F(F(F(F(mvp[r] * p[0]) + F(mvp[4 + r] * p[1])) + F(mvp[8 + r] * p[2])) + F(mvp[12 + r] * F(1)))
                 for r in range(4))


def _inside_r3(c):
    x, y, z, w = c
    return bool(w > 0 and z >= 0 and z <= w)


def _r4(x, y, w, width, height):
    """-> (X, Y, in_guard)"""
    xf = F(F(F(F(F(x / w) * F(0.5)) + F(0.5)) * F(width)) * F(256))
    yf = F(F(F(F(F(y / w) * F(-0.5)) + F(0.5)) * F(height)) * F(256))
    ok = bool(abs(xf) < F(2 ** 23) and abs(yf) < F(2 ** 23))
    return (int(np.rint(xf)), int(np.rint(yf)), True) if ok else (0, 0, False)


def _vertex(c, width, height):
    """(X, Y, d, in_guard) of clip coordinates that pass R3"""
    X, Y, ok = _r4(c[0], c[1], c[3], width, height)
    return X, Y, F(c[2] / c[3]), ok


def _new_vertex(i, o, width, height):
    """N(i, o) of R3c, or None: the whole triangle is clip_skipped"""
    b_i, b_o = F(i[3] - i[2]), F(o[3] - o[2])
    den = F(b_i - b_o)
    if not den > 0:
        return None
    t = F(b_i / den)
    x, y, w = (F(i[k] + F(t * F(o[k] - i[k]))) for k in (0, 1, 3))
    if not w > 0:
        return None
    X, Y, ok = _r4(x, y, w, width, height)
    return X, Y, F(1.0), ok


def pieces_of(c, width, height):
    """R3c of three clip-space vertices -> (list of pieces, form); a piece is three (X, Y, d, in_guard).  form: "whole"
    (R3 accepts it: one piece, the triangle), "skipped" (no piece), "one_in" (one piece) or "one_out" (two)."""
    ins = [_inside_r3(v) for v in c]
    if all(ins):
        return [tuple(_vertex(v, width, height) for v in c)], "whole"
    finite = all(math.isfinite(float(q)) for v in c for q in v)
    if not (finite and all(v[2] >= 0 for v in c) and any(ins)):
        return [], "skipped"
    if sum(ins) == 1:
        k = ins.index(True)
        a, b, cc = c[k], c[(k + 1) % 3], c[(k + 2) % 3]
        nb, nc = _new_vertex(a, b, width, height), _new_vertex(a, cc, width, height)
        if nb is None or nc is None:
            return [], "skipped"
        return [(_vertex(a, width, height), nb, nc)], "one_in"
    k = ins.index(False)
    a, b, cc = c[k], c[(k + 1) % 3], c[(k + 2) % 3]
    p, q = _new_vertex(b, a, width, height), _new_vertex(cc, a, width, height)
    if p is None or q is None:
        return [], "skipped"
    vb, vc = _vertex(b, width, height), _vertex(cc, width, height)
    return [(vb, vc, q), (vb, q, p)], "one_out"


def _draw_piece(piece, width, height, cull_none, vis, ident, extras):
    """R4's guard test and R5-R8 / V2 of one triangle -> (one of PRIORITY, fragments)"""
    if not all(v[3] for v in piece):
        return "guard_skipped", 0
    (x0, y0, d0, _), (x1, y1, d1, _), (x2, y2, d2, _) = piece
    area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    if area == 0:
        return "no_coverage", 0
    if area > 0 and not cull_none:
        return "back_facing", 0
    if area < 0:
        x1, y1, d1, x2, y2, d2, area = x2, y2, d2, x1, y1, d1, -area
    tx, ty = (x0, x1, x2), (y0, y1, y2)
    x_lo, x_hi = max(-((128 - min(tx)) // 256), 0), min((max(tx) - 128) // 256, width - 1)
    y_lo, y_hi = max(-((128 - min(ty)) // 256), 0), min((max(ty) - 128) // 256, height - 1)
    if x_lo > x_hi or y_lo > y_hi:
        return "no_coverage", 0
    extras["lane_pieces" if (x_hi - x_lo + 1) * (y_hi - y_lo + 1) <= 16 else "wave_pieces"] += 1
    px = (256 * np.arange(x_lo, x_hi + 1, dtype=np.int64) + 128)[None, :]
    py = (256 * np.arange(y_lo, y_hi + 1, dtype=np.int64) + 128)[:, None]
    inside = np.ones((y_hi - y_lo + 1, x_hi - x_lo + 1), bool)
    for u, v in ((0, 1), (1, 2), (2, 0)):
        dx, dy = tx[v] - tx[u], ty[v] - ty[u]
        e = dx * (py - ty[u]) - dy * (px - tx[u])
        inside &= (e >= 0) if (dy < 0 or (dy == 0 and dx > 0)) else (e > 0)
    if not inside.any():
        return "no_coverage", 0
    d10, d20, area_f = F(d1 - d0), F(d2 - d0), F(float(area))
    gx = F(F(F(d10 * F(ty[2] - ty[0])) - F(d20 * F(ty[1] - ty[0]))) / area_f)
    gy = F(F(F(d20 * F(tx[1] - tx[0])) - F(d10 * F(tx[2] - tx[0]))) / area_f)
    dd = (d0 + gx * (px - tx[0]).astype(F)) + gy * (py - ty[0]).astype(F)
    assert dd.dtype == F
    dd = np.where(F(1) < dd, F(1), dd)
    write = inside & (dd > 0)
    word = (dd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(ident)
    view = vis[y_lo:y_hi + 1, x_lo:x_hi + 1]
    view[write] = np.maximum(view[write], word[write])
    return "drawn", int(write.sum())


def raster(words, max_commands, meshlet_data, vertices, vertex_count, entity_data, view_proj, width, height,
           visibility=None, command_base=0, flags=CLEAR, vertex_stride=12, position_offset=0, entity_count=None,
           meshlet_data_words=None, max_triangles=256):
    """-> (visibility uint64 (height, width), stats dict, command_error list, extras dict).  max_triangles: V3's limit;
    None restates the depth call, whose result is depth_of() of the words.  extras: `one_in` / `one_out` = triangles
    cut into one / two pieces; `lane_pieces` / `wave_pieces` = pieces (whole triangles included) whose box holds <= 16
    / more samples; `both_routes` = two-piece triangles with one piece of each."""
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
    clip_near, cull_none = bool(flags & CLIP_NEAR), bool(flags & CULL_NONE)
    st = dict.fromkeys(STAT_NAMES, 0)
    extras = dict(one_in=0, one_out=0, lane_pieces=0, wave_pieces=0, both_routes=0)
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
                c = [clips[k] for k in tri]
                if clip_near:
                    pieces, form = pieces_of(c, width, height)
                else:
                    whole = all(_inside_r3(v) for v in c)
                    pieces, form = ([tuple(_vertex(v, width, height) for v in c)], "whole") if whole else ([], "skipped")
                if not pieces:
                    st["clip_skipped"] += 1
                    continue
                if form != "whole":
                    extras[form] += 1
                before = extras["lane_pieces"], extras["wave_pieces"]
                ident = (command_base + i) << 8 | (t & 255)
                results = [_draw_piece(p, width, height, cull_none, vis, ident, extras) for p in pieces]
                if len(pieces) == 2 and (extras["lane_pieces"] - before[0], extras["wave_pieces"] - before[1]) == (1, 1):
                    extras["both_routes"] += 1
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
                 depth=None, flags=CLEAR, **kw):
    """The depth call restated -> (depth float32 (height, width), stats, errors, extras)."""
    loaded = None if depth is None else np.asarray(depth, F).reshape(height, width).view(np.uint32).astype(np.uint64) << np.uint64(32)
    vis, st, errors, extras = raster(words, max_commands, meshlet_data, vertices, vertex_count, entity_data, view_proj,
                                     width, height, visibility=loaded, flags=flags, max_triangles=None, **kw)
    return depth_of(vis), st, errors, extras
