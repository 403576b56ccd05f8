"""An independent numpy restatement of orbit_raster_depth's definition (include/orbit_abi_ext.h R1-R9): np.float32
arithmetic step by step (every product and sum rounded on its own), int64 edge functions evaluated at every sample of a
triangle's box.  It shares no code with the library: tests/test_raster_depth_cpu.py holds the host mirror to it, and
tests/raster_cases.py reads from it what a case exercises."""
import numpy as np

F = np.float32
STAT_NAMES = ("commands", "triangles", "clip_skipped", "guard_skipped", "back_facing", "no_coverage", "fragments",
              "range_errors")
CLEAR, CULL_NONE = 1, 2


def _mat_mul(a, b):
    """OpMatrixTimesMatrix on column-major float32[16]: left-to-right rounded sums."""
    out = np.zeros(16, F)
    for c in range(4):
        for r in range(4):
            out[4 * c + r] = F(F(F(F(a[r] * b[4 * c]) + F(a[4 + r] * b[4 * c + 1])) + F(a[8 + r] * b[4 * c + 2]))
                               + F(a[12 + r] * b[4 * c + 3]))
    return out


def raster(words, max_commands, meshlet_data, vertices, vertex_count, entity_data, view_proj, width, height, depth=None,
           flags=CLEAR, vertex_stride=12, position_offset=0, entity_count=None, meshlet_data_words=None):
    """-> (depth float32 (height, width), stats dict, command_error list, extras dict).  extras: `max_unclamped` = the
    largest interpolated depth of an inside sample before min(d, 1); `nonpositive` = inside samples with !(d > 0);
    `lane_triangles` / `wave_triangles` = drawn triangles whose box holds <= 16 / more samples."""
    words = np.ascontiguousarray(words).view(np.uint8).reshape(-1).view(np.uint32)
    data = np.ascontiguousarray(meshlet_data, dtype=np.uint32).reshape(-1)
    data_words = len(data) if meshlet_data_words is None else meshlet_data_words
    data_bytes = data.view(np.uint8)
    vb = np.ascontiguousarray(vertices).view(np.uint8).reshape(-1)
    ent = np.ascontiguousarray(entity_data).view(np.uint8).reshape(-1).view(F).reshape(-1, 32)
    entity_count = len(ent) if entity_count is None else entity_count
    vp = np.asarray(view_proj, F).reshape(16)
    out = np.zeros((height, width), F) if flags & CLEAR else np.array(depth, F).reshape(height, width).copy()
    bits = out.view(np.uint32)
    st = dict.fromkeys(STAT_NAMES, 0)
    extras = dict(max_unclamped=-np.inf, nonpositive=0, lane_triangles=0, wave_triangles=0)
    errors = []
    count = min(int(words[0]), max_commands)
    old = np.seterr(all="ignore")
    try:
        for i in range(count):
            index_count, _, first_index, index_base, entity, vertex_base, _ = (int(w) for w in words[1 + 7 * i:8 + 7 * i])
            nt, first_word = index_count // 3, first_index // 4
            vcount = first_word - index_base
            st["commands"] += 1
            bad = (first_word < index_base or vcount > 255 or first_word > data_words
                   or (first_index + 3 * nt + 3) // 4 > data_words or entity >= entity_count)
            if not bad:
                gv = vertex_base + data[index_base:index_base + vcount].astype(np.int64)
                corners = data_bytes[first_index:first_index + 3 * nt].reshape(nt, 3).astype(np.int64)
                bad = bool((gv >= vertex_count).any() or (corners >= vcount).any())
            errors.append(int(bad))
            if bad:
                st["range_errors"] += 1
                continue
            st["triangles"] += nt
            if nt == 0:
                continue
            mvp = _mat_mul(vp, ent[entity][:16])
            pos = np.stack([vb[g * vertex_stride + position_offset:g * vertex_stride + position_offset + 12].view(F)
                            for g in gv]) if vcount else np.zeros((0, 3), F)
            x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
            clip = [((mvp[r] * x + mvp[4 + r] * y) + mvp[8 + r] * z) + mvp[12 + r] * F(1) for r in range(4)]
            cx, cy, cz, cw = clip
            clip_ok = (cw > 0) & (cz >= 0) & (cz <= cw)
            d = cz / cw
            xf = ((cx / cw) * F(0.5) + F(0.5)) * F(width) * F(256)
            yf = ((cy / cw) * F(-0.5) + F(0.5)) * F(height) * F(256)
            guard_ok = (np.abs(xf) < F(2 ** 23)) & (np.abs(yf) < F(2 ** 23))
            X = np.where(guard_ok, np.rint(np.where(guard_ok, xf, 0)), 0).astype(np.int64)
            Y = np.where(guard_ok, np.rint(np.where(guard_ok, yf, 0)), 0).astype(np.int64)
            for c0, c1, c2 in corners:
                if not (clip_ok[c0] and clip_ok[c1] and clip_ok[c2]):
                    st["clip_skipped"] += 1
                    continue
                if not (guard_ok[c0] and guard_ok[c1] and guard_ok[c2]):
                    st["guard_skipped"] += 1
                    continue
                area = (X[c1] - X[c0]) * (Y[c2] - Y[c0]) - (X[c2] - X[c0]) * (Y[c1] - Y[c0])
                if area == 0:
                    st["no_coverage"] += 1
                    continue
                if area > 0 and not flags & CULL_NONE:
                    st["back_facing"] += 1
                    continue
                if area < 0:
                    c1, c2, area = c2, c1, -area
                tx, ty = (int(X[c0]), int(X[c1]), int(X[c2])), (int(Y[c0]), int(Y[c1]), int(Y[c2]))
                x_lo, x_hi = max(-((128 - min(tx)) // 256), 0), min((max(tx) - 128) // 256, width - 1)
                y_lo, y_hi = max(-((128 - min(ty)) // 256), 0), min((max(ty) - 128) // 256, height - 1)
                if x_lo > x_hi or y_lo > y_hi:
                    st["no_coverage"] += 1
                    continue
                if (x_hi - x_lo + 1) * (y_hi - y_lo + 1) <= 16:
                    extras["lane_triangles"] += 1
                else:
                    extras["wave_triangles"] += 1
                px = (256 * np.arange(x_lo, x_hi + 1, dtype=np.int64) + 128)[None, :]
                py = (256 * np.arange(y_lo, y_hi + 1, dtype=np.int64) + 128)[:, None]
                inside = np.ones((y_hi - y_lo + 1, x_hi - x_lo + 1), bool)
                for a, b in ((0, 1), (1, 2), (2, 0)):
                    dx, dy = tx[b] - tx[a], ty[b] - ty[a]
                    e = dx * (py - ty[a]) - dy * (px - tx[a])
                    inside &= (e > 0) | ((e == 0) & (dy < 0 or (dy == 0 and dx > 0)))
                if not inside.any():
                    st["no_coverage"] += 1
                    continue
                d0, d1, d2 = d[c0], d[c1], d[c2]
                area_f = F(float(area))
                gx = (F(d1 - d0) * F(ty[2] - ty[0]) - F(d2 - d0) * F(ty[1] - ty[0])) / area_f
                gy = (F(d2 - d0) * F(tx[1] - tx[0]) - F(d1 - d0) * F(tx[2] - tx[0])) / area_f
                dd = (d0 + gx * (px - tx[0]).astype(F)) + gy * (py - ty[0]).astype(F)
                assert dd.dtype == F
                if np.isfinite(dd[inside]).any():
                    extras["max_unclamped"] = max(extras["max_unclamped"], float(np.nanmax(dd[inside])))
                dd = np.where(F(1) < dd, F(1), dd)
                write = inside & (dd > 0)
                extras["nonpositive"] += int((inside & ~write).sum())
                st["fragments"] += int(write.sum())
                view = bits[y_lo:y_hi + 1, x_lo:x_hi + 1]
                view[write] = np.maximum(view[write], dd.view(np.uint32)[write])
    finally:
        np.seterr(**old)
    return out, st, errors, extras
