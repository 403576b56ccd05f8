"""An independent numpy restatement of orbit_visibility_surface (include/orbit_abi_ext.h S1-S7 over R1-R7 and R9): its own
decode of the words and of the commands, np.float32 arithmetic step by step (every operation rounded on its own), exact
integers for the edge values — Python integers per triangle, int64 arrays over a triangle's pixels, each value below
2^50 and so exact in either — and the (float)(double) conversion spelled out.  It shares no code with the library or with
the host mirror and does not load them: tests/test_visibility_surface_cpu.py holds the mirror to it.

The work is grouped per distinct (command, triangle): everything S2 asks of the triangle once, then S3-S5 on the array of
its pixels.  That is an arrangement, not a shortcut: every pixel goes through every rule."""
import numpy as np

F = np.float32
CLEAR = 1
E_RANGE = -9
MAX_COMMANDS = 1 << 24
STAT_NAMES = ("covered_pixels", "written_pixels", "foreign_pixels", "unsupported_pixels", "stale_pixels", "degenerate_pixels")


def _mvp(a, b):
    """R2: OpMatrixTimesMatrix on column-major float32[16], left-to-right rounded sums."""
    out = np.zeros(16, F)
    for c in range(4):
        for r in range(4):
            acc = F(a[r] * b[4 * c])
            for k in (1, 2, 3):
                acc = F(acc + F(a[4 * k + r] * b[4 * c + k]))
            out[4 * c + r] = acc
    return out


def _command(words, k, data, corner_bytes, data_words, entity_count, vertex_count):
    """R1's decode and R9 / V3 of command k -> None (it fails) or (nt, first_index, index_base, entity, vertex_base)."""
    index_count, _, first_index, index_base, entity, vertex_base, _ = (int(w) for w in words[1 + 7 * k:8 + 7 * k])
    nt, first_word = index_count // 3, first_index // 4
    vcount = first_word - index_base
    if (first_word < index_base or vcount > 255 or first_word > data_words or (first_index + 3 * nt + 3) // 4 > data_words
            or entity >= entity_count or nt > 256):
        return None
    if (vertex_base + data[index_base:index_base + vcount].astype(np.int64) >= vertex_count).any():
        return None
    if (corner_bytes[first_index:first_index + 3 * nt] >= vcount).any():
        return None
    return nt, first_index, index_base, entity, vertex_base


def _bary(tx, ty, iw, swapped, px, py):
    """S3 at the samples (px, py) (int64 arrays) of the normalised triangle -> (l1, l2, s > 0), corner order restored."""
    e = []
    for u, v in ((0, 1), (1, 2), (2, 0)):
        dx, dy = tx[v] - tx[u], ty[v] - ty[u]
        raw = dx * (py - ty[u]) - dy * (px - tx[u])  # int64, exact
        assert np.abs(raw).max(initial=0) < 2 ** 52
        e.append(raw.astype(np.float64).astype(F))
    q0, q1, q2 = e[1] * iw[0], e[2] * iw[1], e[0] * iw[2]
    s = (q0 + q1) + q2
    l1, l2 = q1 / s, q2 / s
    assert l1.dtype == F and s.dtype == F
    return (l2, l1, s > 0) if swapped else (l1, l2, s > 0)


def surface(visibility, words, max_commands, meshlet_data, vertices, vertex_count, entity_data, view_proj, command_base=0,
            clear=True, into=None, want=("bary", "grad", "triangle"), vertex_stride=12, position_offset=0, entity_count=None,
            meshlet_data_words=None, fill=0):
    """-> dict(bary (h, w, 2) float32, grad (h, w, 4) float32, triangle (h, w, 4) uint32 (None unless in `want`), stats:
    dict, status).  The arguments are orbit_amd.raster.host_visibility_surface's."""
    assert command_base + max_commands <= MAX_COMMANDS
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
    commands = {}
    old = np.seterr(all="ignore")
    try:
        for key in np.unique(low):
            sel = low == key
            y, x, hi = ys[sel], xs[sel], high[sel]
            count = int(sel.sum())
            k, t = (int(key) >> 8) - command_base, int(key) & 255
            if k not in commands:
                commands[k] = _command(words, k, data, corner_bytes, data_words, entity_count, vertex_count)
            # S2
            if commands[k] is None or t >= commands[k][0]:
                st["stale_pixels"] += count
                continue
            nt, first_index, index_base, entity, vertex_base = commands[k]
            corners = [int(c) for c in corner_bytes[first_index + 3 * t:first_index + 3 * t + 3]]
            g = [vertex_base + int(data[index_base + c]) for c in corners]
            mvp = _mvp(vp, ent[entity][:16])
            cw, d, X, Y, ok = [], [], [], [], True
            for gv in g:
                px_, py_, pz_ = vb[gv * vertex_stride + position_offset:][:12].view(F)
                cx, cy, cz, w = (F(F(F(mvp[r] * px_) + F(mvp[4 + r] * py_)) + F(mvp[8 + r] * pz_)) + F(mvp[12 + r] * F(1))
                                 for r in range(4))
                cx, cy, cz, w = F(cx), F(cy), F(cz), F(w)
                xf = F(F(F(F(F(cx / w) * F(0.5)) + F(0.5)) * F(width)) * F(256))
                yf = F(F(F(F(F(cy / w) * F(-0.5)) + F(0.5)) * F(height)) * F(256))
                ok = ok and bool(w > 0 and cz >= 0 and cz <= w) and bool(abs(xf) < F(2 ** 23) and abs(yf) < F(2 ** 23))
                cw.append(w), d.append(F(cz / w))
                X.append(int(np.rint(xf)) if np.isfinite(xf) else 0), Y.append(int(np.rint(yf)) if np.isfinite(yf) else 0)
            if not ok:
                st["unsupported_pixels"] += count
                continue
            a, b, c = 0, 1, 2
            area = (X[b] - X[a]) * (Y[c] - Y[a]) - (X[c] - X[a]) * (Y[b] - Y[a])
            swapped = area < 0
            if swapped:
                b, c, area = c, b, -area
            tx, ty = [X[a], X[b], X[c]], [Y[a], Y[b], Y[c]]
            x_lo, x_hi = max(-((128 - min(tx)) // 256), 0), min((max(tx) - 128) // 256, width - 1)
            y_lo, y_hi = max(-((128 - min(ty)) // 256), 0), min((max(ty) - 128) // 256, height - 1)
            if area == 0 or x_lo > x_hi or y_lo > y_hi:
                st["stale_pixels"] += count
                continue
            px, py = 256 * x.astype(np.int64) + 128, 256 * y.astype(np.int64) + 128
            inside = np.ones(count, bool)
            for u, v in ((0, 1), (1, 2), (2, 0)):
                dx, dy = tx[v] - tx[u], ty[v] - ty[u]
                e = dx * (py - ty[u]) - dy * (px - tx[u])
                inside &= (e >= 0) if (dy < 0 or (dy == 0 and dx > 0)) else (e > 0)
            d10, d20, area_f = F(d[b] - d[a]), F(d[c] - d[a]), F(float(area))
            gx = F(F(F(d10 * F(ty[2] - ty[0])) - F(d20 * F(ty[1] - ty[0]))) / area_f)
            gy = F(F(F(d20 * F(tx[1] - tx[0])) - F(d10 * F(tx[2] - tx[0]))) / area_f)
            dd = (d[a] + gx * (px - tx[0]).astype(F)) + gy * (py - ty[0]).astype(F)
            assert dd.dtype == F
            dd = np.where(F(1) < dd, F(1), dd)
            good = inside & (dd > 0) & (dd.view(np.uint32) == hi)
            st["stale_pixels"] += int((~good).sum())
            y, x, px, py, count = y[good], x[good], px[good], py[good], int(good.sum())
            if count == 0:
                continue
            # S3, S4
            iw = [F(F(1) / cw[a]), F(F(1) / cw[b]), F(F(1) / cw[c])]
            l1, l2, _ = _bary(tx, ty, iw, swapped, px, py)
            l1x, l2x, pos_x = _bary(tx, ty, iw, swapped, px + 256, py)
            l1y, l2y, pos_y = _bary(tx, ty, iw, swapped, px, py + 256)
            zero = np.zeros(count, F)
            six = np.stack([l1, l2, np.where(pos_x, l1x - l1, zero), np.where(pos_x, l2x - l2, zero),
                            np.where(pos_y, l1y - l1, zero), np.where(pos_y, l2y - l2, zero)], axis=1)
            assert six.dtype == F
            # S5
            finite = np.isfinite(six)
            six = np.where(finite, six, F(0))
            st["written_pixels"] += count
            st["degenerate_pixels"] += int((~finite.all(axis=1) | ~pos_x | ~pos_y).sum())
            if outs["bary"] is not None:
                outs["bary"][y, x] = six[:, :2]
            if outs["grad"] is not None:
                outs["grad"][y, x] = six[:, 2:]
            if outs["triangle"] is not None:  # S6
                outs["triangle"][y, x] = np.array([entity] + [gv & 0xFFFFFFFF for gv in g], np.uint32)
    finally:
        np.seterr(**old)
    return dict(outs, stats=st, status=E_RANGE if st["stale_pixels"] else 0)
