"""An independent numpy / Python-integer restatement of orbit_visibility_surface_drawn (include/orbit_abi_ext.h S1, S2d,
S3, S3w, S3c, S4-S7 over R1-R7, R3c, R4w-R7w and R9): its own decode of the words, its own cut at the near plane, its own
wide integers (Python integers, exact at any size), np.float32 / np.float64 steps in the stated order with every
operation rounded on its own.  It shares no code with the library, with surface_common.h or with the host mirror and
does not load them: tests/test_surface_drawn_cpu.py holds the mirror to it.  (R2's matrix product and R9's command check
are the ones tests/visibility_surface_ref.py restates; they are test code too.)

The work is grouped per distinct (command, triangle): the class of the key and its candidates once, then the pixels of
the key as arrays — int64 arrays for a narrow candidate, object arrays of Python integers for a wide one.  That is an
arrangement, not a shortcut: every pixel goes through every rule.  Beside the outputs the restatement keeps, per written
pixel, what the accuracy and reprojection checks need: `detail[(y, x)]` is filled on request (`keep_detail`)."""
from fractions import Fraction

import numpy as np

from visibility_surface_ref import _command, _mvp

F, D = np.float32, np.float64
CLEAR = 1
CLIP, WIDE = 8, 32  # ORBIT_RASTER_CLIP_NEAR, ORBIT_RASTER_WIDE_GUARD
E_RANGE = -9
MAX_COMMANDS = 1 << 24
STAT_NAMES = ("covered_pixels", "written_pixels", "foreign_pixels", "unsupported_pixels", "stale_pixels", "degenerate_pixels",
              "cut_pixels", "wide_pixels")
NARROW, GUARD_FAIL, WIDE_VERTEX, OUT_OF_BAND = range(4)
M64 = (1 << 64) - 1


def clip_in(c):
    return bool(c[3] > 0 and c[2] >= 0 and c[2] <= c[3])


def snap(c, width, height, wide, near=False):
    """R3-R4 / R4w of clip coordinates c = (x, y, z, w) -> (X, Y, depth, kind); `near`: a new vertex of R3c, depth 1"""
    x, y, z, w = c
    xf = F(F(F(F(F(x / w) * F(0.5)) + F(0.5)) * F(width)) * F(256))
    yf = F(F(F(F(F(y / w) * F(-0.5)) + F(0.5)) * F(height)) * F(256))
    d = F(1) if near else F(z / w)
    if abs(xf) < F(2 ** 23) and abs(yf) < F(2 ** 23):
        return int(np.rint(xf)), int(np.rint(yf)), d, NARROW
    if not wide:
        return 0, 0, d, GUARD_FAIL
    if abs(xf) < F(2 ** 60) and abs(yf) < F(2 ** 60):
        return int(np.rint(xf)), int(np.rint(yf)), d, WIDE_VERTEX
    return 0, 0, d, OUT_OF_BAND


def corner(c, k, width, height, wide):
    """an original corner as a piece vertex: (clip w, weights over the original corners, snap)"""
    m = [F(0)] * 3
    m[k] = F(1)
    return dict(w=c[3], m=m, t=None, io=(k, k), snap=snap(c, width, height, wide))


def new_vertex(clips, i, o, width, height, wide):
    """R3c's N(i, o) -> None (the triangle stays clip_skipped) or the piece vertex"""
    ci, co = clips[i], clips[o]
    b_i, b_o = F(ci[3] - ci[2]), F(co[3] - co[2])
    den = F(b_i - b_o)
    if not den > 0:
        return None
    t = F(b_i / den)
    x = F(ci[0] + F(t * F(co[0] - ci[0])))
    y = F(ci[1] + F(t * F(co[1] - ci[1])))
    w = F(ci[3] + F(t * F(co[3] - ci[3])))
    if not w > 0:
        return None
    m = [F(0)] * 3
    m[i], m[o] = F(F(1) - t), t
    return dict(w=w, m=m, t=t, io=(i, o), snap=snap((x, y, F(0), w), width, height, wide, near=True))


def pieces_of(clips, width, height, wide):
    """R3c -> the pieces, each three piece vertices, in R3c's order; [] if the triangle stays clip_skipped"""
    ins = [clip_in(c) for c in clips]
    if sum(ins) in (0, 3):
        return []
    if not all(np.isfinite(v) for c in clips for v in c) or not all(c[2] >= 0 for c in clips):
        return []
    if sum(ins) == 1:
        a = ins.index(True)
        b, c = (a + 1) % 3, (a + 2) % 3
        n0, n1 = new_vertex(clips, a, b, width, height, wide), new_vertex(clips, a, c, width, height, wide)
        if n0 is None or n1 is None:
            return []
        return [[corner(clips[a], a, width, height, wide), n0, n1]]
    a = ins.index(False)
    b, c = (a + 1) % 3, (a + 2) % 3
    q, p = new_vertex(clips, c, a, width, height, wide), new_vertex(clips, b, a, width, height, wide)
    if q is None or p is None:
        return []
    vb, vc = corner(clips[b], b, width, height, wide), corner(clips[c], c, width, height, wide)
    return [[vb, vc, q], [vb, q, p]]


def make_setup(verts, width, height):
    """R5-R7 / R5w-R7w of three piece vertices (none out of band or guard-failing without WIDE), the facing not asked
    -> None (no area, empty box) or the setup: normalised order, integer vertices, the depth plane"""
    is_wide = any(v["snap"][3] == WIDE_VERTEX for v in verts)
    X, Y, d = [v["snap"][0] for v in verts], [v["snap"][1] for v in verts], [v["snap"][2] for v in verts]
    order = [0, 1, 2]
    area = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
    if area == 0:
        return None
    if area < 0:
        order, area = [0, 2, 1], -area
    tx, ty, td = [X[i] for i in order], [Y[i] for i in order], [d[i] for i in order]
    x_lo, x_hi = max(-((128 - min(tx)) // 256), 0), min((max(tx) - 128) // 256, width - 1)
    y_lo, y_hi = max(-((128 - min(ty)) // 256), 0), min((max(ty) - 128) // 256, height - 1)
    if x_lo > x_hi or y_lo > y_hi:
        return None
    if is_wide:
        area_d = D(float(area >> 64)) * D(2.0 ** 64) + D(float(area & M64))
        d10, d20 = D(td[1]) - D(td[0]), D(td[2]) - D(td[0])
        gx = (d10 * D(float(ty[2] - ty[0])) - d20 * D(float(ty[1] - ty[0]))) / area_d
        gy = (d20 * D(float(tx[1] - tx[0])) - d10 * D(float(tx[2] - tx[0]))) / area_d
        plane = (D(td[0]), gx, gy)
    else:
        area_f = F(float(area))
        d10, d20 = F(td[1] - td[0]), F(td[2] - td[0])
        gx = F(F(F(d10 * F(ty[2] - ty[0])) - F(d20 * F(ty[1] - ty[0]))) / area_f)
        gy = F(F(F(d20 * F(tx[1] - tx[0])) - F(d10 * F(tx[2] - tx[0]))) / area_f)
        plane = (td[0], gx, gy)
    return dict(order=order, tx=tx, ty=ty, plane=plane, wide=is_wide, verts=verts)


def edge_values(s, px, py):
    """E_j (without the bias) of the normalised edges j = 0, 1, 2 at the samples: int64 arrays, or object arrays of
    Python integers for a wide setup"""
    tx, ty = s["tx"], s["ty"]
    if s["wide"]:
        px, py = px.astype(object), py.astype(object)
    out = []
    for u, v in ((0, 1), (1, 2), (2, 0)):
        dx, dy = tx[v] - tx[u], ty[v] - ty[u]
        e = dx * (py - ty[u]) - dy * (px - tx[u])
        if not s["wide"]:
            assert np.abs(e).max(initial=0) < 2 ** 52
        out.append(e)
    return out


def edge_floats(s, raw):
    """S3 / S3w: e_j as float32"""
    if not s["wide"]:
        return [e.astype(D).astype(F) for e in raw]
    return [np.array([D(float(int(v) >> 64)) * D(2.0 ** 64) + D(float(int(v) & M64)) for v in e], D).astype(F) for e in raw]


def owned(s, px, py, high):
    """S2d: inside (top-left rule) and the depth > 0 and bit-equal to the word's high half"""
    tx, ty = s["tx"], s["ty"]
    raw = edge_values(s, px, py)
    inside = np.ones(len(px), bool)
    for (u, v), e in zip(((0, 1), (1, 2), (2, 0)), raw):
        dx, dy = tx[v] - tx[u], ty[v] - ty[u]
        top_left = dy < 0 or (dy == 0 and dx > 0)
        inside &= np.array([(q >= 0) if top_left else (q > 0) for q in e], bool) if s["wide"] else ((e >= 0) if top_left else (e > 0))
    d0, gx, gy = s["plane"]
    if s["wide"]:
        ddx = np.array([float(int(q) - tx[0]) for q in px], D)
        ddy = np.array([float(int(q) - ty[0]) for q in py], D)
        dd = ((d0 + gx * ddx) + gy * ddy).astype(F)
    else:
        dd = (d0 + gx * (px - tx[0]).astype(F)) + gy * (py - ty[0]).astype(F)
        assert dd.dtype == F
    dd = np.where(F(1) < dd, F(1), dd)
    return inside & (dd > 0) & (dd.view(np.uint32) == high)


def bary(s, cut, px, py):
    """S3, S3w or S3c at the samples -> (l1, l2, s > 0) in meshlet_data's corner order"""
    e = edge_floats(s, edge_values(s, px, py))
    verts, order = s["verts"], s["order"]
    Q = [None] * 3
    for j in range(3):  # normalised vertex j is piece vertex order[j]; its q takes the edge opposite: j + 1
        i = order[j]
        Q[i] = e[(j + 1) % 3] * F(F(1) / verts[i]["w"])
        assert Q[i].dtype == F
    if not cut:  # the piece vertices ARE the corners, in order
        total = (Q[order[0]] + Q[order[1]]) + Q[order[2]]
        l1n, l2n = Q[order[1]] / total, Q[order[2]] / total
        return (l2n, l1n, total > 0) if order[1] == 2 else (l1n, l2n, total > 0)
    n = [(Q[0] * verts[0]["m"][c] + Q[1] * verts[1]["m"][c]) + Q[2] * verts[2]["m"][c] for c in range(3)]
    total = (n[0] + n[1]) + n[2]
    assert total.dtype == F
    return n[1] / total, n[2] / total, total > 0


def surface(visibility, words, max_commands, meshlet_data, vertices, vertex_count, entity_data, view_proj, command_base=0,
            clear=True, into=None, want=("bary", "grad", "triangle"), vertex_stride=12, position_offset=0, entity_count=None,
            meshlet_data_words=None, fill=0, raster_flags=0, keep_detail=False):
    """-> dict(bary, grad, triangle (None unless in `want`), stats: dict, status, detail).  The arguments are
    orbit_amd.raster.host_visibility_surface_drawn's.  detail (keep_detail): owner (h, w): the index into `setups` =
    [(setup, cut, clips)] of each written pixel's candidate, -1 elsewhere; approx (h, w, 2): approx_lambdas of the same;
    owned_by_two: the pixels both pieces of a cut triangle own."""
    assert command_base + max_commands <= MAX_COMMANDS and not raster_flags & ~(CLIP | WIDE)
    with_clip, with_wide = bool(raster_flags & CLIP), bool(raster_flags & WIDE)
    vis = np.ascontiguousarray(visibility, dtype=np.uint64)
    height, width = vis.shape
    words = np.ascontiguousarray(words).view(np.uint8).reshape(-1).view(np.uint32)
    data = np.ascontiguousarray(meshlet_data, dtype=np.uint32).reshape(-1)
    data_words = len(data) if meshlet_data_words is None else meshlet_data_words
    corner_bytes = data.view(np.uint8)
    vb = np.ascontiguousarray(vertices).view(np.uint8).reshape(-1)
    ent = np.ascontiguousarray(entity_data).view(np.uint8).reshape(-1).view(F).reshape(-1, 32)
    entity_count = len(ent) if entity_count is None else entity_count
    vp = np.asarray(view_proj, F).reshape(16)
    outs = {}
    for name, per_pixel, dtype, cleared in (("bary", 2, F, 0), ("grad", 4, F, 0), ("triangle", 4, np.uint32, 0xFFFFFFFF)):
        if name not in want:
            outs[name] = None
            continue
        if into is not None:
            a = np.array(into[name], dtype=dtype, order="C").reshape(height, width, per_pixel)
        else:
            a = np.full((height, width, per_pixel), fill, np.uint32).view(dtype)
        if clear:  # S7
            a.view(np.uint32)[:] = cleared
        outs[name] = a
    st = dict.fromkeys(STAT_NAMES, 0)
    detail = dict(owner=np.full((height, width), -1, np.int32), setups=[], approx=np.zeros((height, width, 2), D), owned_by_two=0)
    n = min(int(words[0]), max_commands)
    # S1
    ys, xs = np.nonzero(vis)
    st["covered_pixels"] = len(ys)
    low = (vis[ys, xs] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    high = (vis[ys, xs] >> np.uint64(32)).astype(np.uint32)
    k_all = (low >> 8) - command_base
    own = (k_all >= 0) & (k_all < n)
    st["foreign_pixels"] = int((~own).sum())
    ys, xs, low, high = ys[own], xs[own], low[own], high[own]
    commands, mvps = {}, {}
    old = np.seterr(all="ignore")
    try:
        for key in np.unique(low):
            sel = low == key
            y, x, hi = ys[sel], xs[sel], high[sel]
            count = int(sel.sum())
            k, t = (int(key) >> 8) - command_base, int(key) & 255
            if k not in commands:
                commands[k] = _command(words, k, data, corner_bytes, data_words, entity_count, vertex_count)
            if commands[k] is None or t >= commands[k][0]:
                st["stale_pixels"] += count
                continue
            nt, first_index, index_base, entity, vertex_base = commands[k]
            corners = [int(c) for c in corner_bytes[first_index + 3 * t:first_index + 3 * t + 3]]
            g = [vertex_base + int(data[index_base + c]) for c in corners]
            if entity not in mvps:
                mvps[entity] = _mvp(vp, ent[entity][:16])
            mvp = mvps[entity]
            clips = []
            for gv in g:
                p = vb[gv * vertex_stride + position_offset:][:12].view(F)
                clips.append(tuple(F(F(F(F(mvp[r] * p[0]) + F(mvp[4 + r] * p[1])) + F(mvp[8 + r] * p[2])) + F(mvp[12 + r] * F(1)))
                                   for r in range(4)))
            # S2d: the class, its candidates [(three piece vertices, cut)] and what a pixel none of them owns is
            miss, candidates = "stale_pixels", []
            if all(clip_in(c) for c in clips):
                verts = [corner(c, q, width, height, with_wide) for q, c in enumerate(clips)]
                kinds = {v["snap"][3] for v in verts}
                if GUARD_FAIL in kinds:  # (b) without WIDE
                    miss = "unsupported_pixels"
                elif OUT_OF_BAND not in kinds:  # (a), or (b) with WIDE
                    candidates = [(verts, False)]
            elif not with_clip:  # (c) without CLIP
                miss = "unsupported_pixels"
            else:
                for verts in pieces_of(clips, width, height, with_wide):
                    kinds = {v["snap"][3] for v in verts}
                    if OUT_OF_BAND in kinds:
                        continue
                    if GUARD_FAIL in kinds:
                        miss = "unsupported_pixels"
                        continue
                    candidates.append((verts, True))
            px, py = 256 * x.astype(np.int64) + 128, 256 * y.astype(np.int64) + 128
            left = np.ones(count, bool)
            for verts, cut in candidates:
                if not left.any():
                    break
                s = make_setup(verts, width, height)
                if s is None:
                    continue
                idx = np.flatnonzero(left)
                good = owned(s, px[idx], py[idx], hi[idx])
                idx = idx[good]
                left[idx] = False
                m = len(idx)
                if m == 0:
                    continue
                # S3, S3w, S3c; S4
                l1, l2, _ = bary(s, cut, px[idx], py[idx])
                l1x, l2x, pos_x = bary(s, cut, px[idx] + 256, py[idx])
                l1y, l2y, pos_y = bary(s, cut, px[idx], py[idx] + 256)
                zero = np.zeros(m, F)
                six = np.stack([l1, l2, np.where(pos_x, l1x - l1, zero), np.where(pos_x, l2x - l2, zero),
                                np.where(pos_y, l1y - l1, zero), np.where(pos_y, l2y - l2, zero)], axis=1)
                assert six.dtype == F
                finite = np.isfinite(six)  # S5
                six = np.where(finite, six, F(0))
                st["written_pixels"] += m
                st["degenerate_pixels"] += int((~finite.all(axis=1) | ~pos_x | ~pos_y).sum())
                st["cut_pixels"] += m if cut else 0
                st["wide_pixels"] += m if s["wide"] else 0
                if outs["bary"] is not None:
                    outs["bary"][y[idx], x[idx]] = six[:, :2]
                if outs["grad"] is not None:
                    outs["grad"][y[idx], x[idx]] = six[:, 2:]
                if outs["triangle"] is not None:  # S6
                    outs["triangle"][y[idx], x[idx]] = np.array([entity] + [gv & 0xFFFFFFFF for gv in g], np.uint32)
                if keep_detail:
                    detail["owner"][y[idx], x[idx]] = len(detail["setups"])
                    detail["setups"].append((s, cut, clips))
                    detail["approx"][y[idx], x[idx]] = approx_lambdas(s, px[idx], py[idx])
            if keep_detail and len(candidates) == 2 and all(make_setup(v, width, height) is not None for v, _ in candidates):
                both = owned(make_setup(candidates[0][0], width, height), px, py, hi) & owned(make_setup(candidates[1][0], width, height), px, py, hi)
                detail["owned_by_two"] += int(both.sum())
            st[miss] += int(left.sum())
    finally:
        np.seterr(**old)
    return dict(outs, stats=st, status=E_RANGE if st["stale_pixels"] else 0, detail=detail)


# ------------------------------------------------------------------------------ the exact value, for the accuracy checks
def approx_lambdas(s, px, py):
    """exact_lambdas in float64 over arrays of samples.  The exact value is a quotient of sums of non-negative terms
    inside the candidate, so float64 (every step within 2^-52, nothing cancels) gives it to better than 2^-47 relative: a
    sieve for the rational check, and a measurement to that accuracy."""
    raw = edge_values(s, px, py)
    e = [np.array([float(int(v)) for v in q], D) if s["wide"] else q.astype(D) for q in raw]
    verts, order = s["verts"], s["order"]
    n = [np.zeros(len(px), D) for _ in range(3)]
    for j in range(3):
        i = order[j]
        q = e[(j + 1) % 3] / D(verts[i]["w"])
        a, b = verts[i]["io"]
        if a == b:
            n[a] = n[a] + q
        else:
            t = D(verts[i]["t"])
            n[a], n[b] = n[a] + q * (D(1) - t), n[b] + q * t
    total = (n[0] + n[1]) + n[2]
    return np.stack([n[1] / total, n[2] / total], axis=1)


def exact_lambdas(s, cut, x, y, affine=False):
    """The exact rational (l1, l2) of pixel (x, y) in the candidate's setup: the snapped integers, and the float values of
    w_i and t taken as exact rationals (a piece: the weights 1 - t and t exact, not the rounded 1.0f - t).  affine: every
    w taken as 1, the screen-space value."""
    px, py = 256 * x + 128, 256 * y + 128
    tx, ty, verts, order = s["tx"], s["ty"], s["verts"], s["order"]
    edge = lambda u, v: (tx[v] - tx[u]) * (py - ty[u]) - (ty[v] - ty[u]) * (px - tx[u])  # noqa: E731
    e = [edge(0, 1), edge(1, 2), edge(2, 0)]
    Q = [None] * 3
    for j in range(3):
        i = order[j]
        Q[i] = Fraction(e[(j + 1) % 3]) / (1 if affine else Fraction(float(verts[i]["w"])))
    n = [Fraction(0)] * 3
    for i, v in enumerate(verts):
        a, b = v["io"]
        if a == b:
            n[a] += Q[i]
        else:
            t = Fraction(float(v["t"]))
            n[a] += Q[i] * (1 - t)
            n[b] += Q[i] * t
    total = sum(n)
    return n[1] / total, n[2] / total
