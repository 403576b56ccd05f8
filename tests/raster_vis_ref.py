"""An independent numpy restatement of orbit_raster_visibility and orbit_visibility_resolve (include/orbit_abi_ext.h
V1-V4 over R1-R9): np.float32 arithmetic step by step, int64 edge functions at every sample of a triangle's box, a
per-pixel u64 maximum of words it builds itself.  It shares no code with the library or with the host mirror:
tests/test_raster_visibility_cpu.py holds the mirror to it."""
import numpy as np

F = np.float32
STAT_NAMES = ("commands", "triangles", "clip_skipped", "guard_skipped", "back_facing", "no_coverage", "fragments",
              "range_errors")
CLEAR, CULL_NONE = 1, 2
MAX_TRIANGLES = 256    # V3
MAX_COMMANDS = 1 << 24


def _mvp(a, b):
    """OpMatrixTimesMatrix on column-major float32[16]: left-to-right rounded sums."""
    out = np.zeros(16, F)
    for c in range(4):
        for r in range(4):
            acc = F(a[r] * b[4 * c])
            for k in (1, 2, 3):
                acc = F(acc + F(a[4 * k + r] * b[4 * c + k]))
            out[4 * c + r] = acc
    return out


def _top_left(dx, dy):
    return dy < 0 or (dy == 0 and dx > 0)


def raster(words, max_commands, meshlet_data, vertices, vertex_count, entity_data, view_proj, width, height,
           visibility=None, command_base=0, flags=CLEAR, vertex_stride=12, position_offset=0, entity_count=None,
           meshlet_data_words=None):
    """-> (visibility uint64 (height, width), stats dict, command_error list, extras dict).  extras: `lane_triangles` /
    `wave_triangles` = drawn triangles whose box holds <= 16 / more samples; `won` = winners() of the result."""
    assert command_base + max_commands <= MAX_COMMANDS
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
    st = dict.fromkeys(STAT_NAMES, 0)
    extras = dict(lane_triangles=0, wave_triangles=0)
    errors = []
    old = np.seterr(all="ignore")
    try:
        for i in range(min(int(words[0]), max_commands)):
            index_count, _, first_index, index_base, entity, vertex_base, _ = (int(w) for w in words[1 + 7 * i:8 + 7 * i])
            nt, first_word = index_count // 3, first_index // 4
            vcount = first_word - index_base
            st["commands"] += 1
            bad = (first_word < index_base or vcount > 255 or first_word > data_words or nt > MAX_TRIANGLES
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
            if nt == 0:
                continue
            command_id = np.uint64((command_base + i) << 8)
            mvp = _mvp(vp, ent[entity][:16])
            pos = np.stack([vb[g * vertex_stride + position_offset:][:12].view(F) for g in gv])
            x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
            cx, cy, cz, cw = (((mvp[r] * x + mvp[4 + r] * y) + mvp[8 + r] * z) + mvp[12 + r] * F(1) for r in range(4))
            visible = (cw > 0) & (cz >= 0) & (cz <= cw)
            d = cz / cw
            xf = ((cx / cw) * F(0.5) + F(0.5)) * F(width) * F(256)
            yf = ((cy / cw) * F(-0.5) + F(0.5)) * F(height) * F(256)
            guarded = (np.abs(xf) < F(2 ** 23)) & (np.abs(yf) < F(2 ** 23))
            X = np.rint(np.where(guarded, xf, 0)).astype(np.int64)
            Y = np.rint(np.where(guarded, yf, 0)).astype(np.int64)
            for t, (a, b, c) in enumerate(corners):
                if not visible[[a, b, c]].all():
                    st["clip_skipped"] += 1
                    continue
                if not guarded[[a, b, c]].all():
                    st["guard_skipped"] += 1
                    continue
                area = int((X[b] - X[a]) * (Y[c] - Y[a]) - (X[c] - X[a]) * (Y[b] - Y[a]))
                if area == 0:
                    st["no_coverage"] += 1
                    continue
                if area > 0:
                    if not flags & CULL_NONE:
                        st["back_facing"] += 1
                        continue
                else:
                    b, c, area = c, b, -area
                tx, ty = [int(X[k]) for k in (a, b, c)], [int(Y[k]) for k in (a, b, c)]
                x_lo, x_hi = max(-((128 - min(tx)) // 256), 0), min((max(tx) - 128) // 256, width - 1)
                y_lo, y_hi = max(-((128 - min(ty)) // 256), 0), min((max(ty) - 128) // 256, height - 1)
                if x_lo > x_hi or y_lo > y_hi:
                    st["no_coverage"] += 1
                    continue
                extras["lane_triangles" if (x_hi - x_lo + 1) * (y_hi - y_lo + 1) <= 16 else "wave_triangles"] += 1
                px = (256 * np.arange(x_lo, x_hi + 1, dtype=np.int64) + 128)[None, :]
                py = (256 * np.arange(y_lo, y_hi + 1, dtype=np.int64) + 128)[:, None]
                inside = np.ones((y_hi - y_lo + 1, x_hi - x_lo + 1), bool)
                for u, v in ((0, 1), (1, 2), (2, 0)):
                    dx, dy = tx[v] - tx[u], ty[v] - ty[u]
                    e = dx * (py - ty[u]) - dy * (px - tx[u])
                    inside &= (e >= 0) if _top_left(dx, dy) else (e > 0)
                if not inside.any():
                    st["no_coverage"] += 1
                    continue
                d10, d20, area_f = F(d[b] - d[a]), F(d[c] - d[a]), F(float(area))
                gx = (d10 * F(ty[2] - ty[0]) - d20 * F(ty[1] - ty[0])) / area_f
                gy = (d20 * F(tx[1] - tx[0]) - d10 * F(tx[2] - tx[0])) / area_f
                dd = (d[a] + gx * (px - tx[0]).astype(F)) + gy * (py - ty[0]).astype(F)
                assert dd.dtype == F
                dd = np.where(F(1) < dd, F(1), dd)
                write = inside & (dd > 0)
                st["fragments"] += int(write.sum())
                # V2: the word is the depth's bits above the command and the triangle
                word = (dd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (command_id | np.uint64(t))
                view = vis[y_lo:y_hi + 1, x_lo:x_hi + 1]
                view[write] = np.maximum(view[write], word[write])
    finally:
        np.seterr(**old)
    extras["won"] = winners(vis, command_base, max_commands)
    return vis, st, errors, extras


def winners(visibility, command_base, max_commands):
    """{(command, triangle): pixels} of the covered pixels whose command lies in [command_base, + max_commands)."""
    vis = np.asarray(visibility, np.uint64)
    ids = (vis[vis != 0] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ids = ids[(ids >> 8 >= command_base) & (ids >> 8 < command_base + max_commands)]
    return {(int(k) >> 8, int(k) & 255): int(n) for k, n in zip(*np.unique(ids, return_counts=True))}


def resolve(visibility, command_base, max_commands):
    """-> (depth float32, command_pixels uint32[max_commands], dict of OrbitVisibilityStats) by counting, not by walking."""
    vis = np.asarray(visibility, np.uint64)
    depth = (vis >> np.uint64(32)).astype(np.uint32).view(F).reshape(vis.shape)
    covered = vis != 0
    command = ((vis >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.int64)
    own = covered & (command >= command_base) & (command < command_base + max_commands)
    pixels = np.bincount(command[own] - command_base, minlength=max_commands).astype(np.uint32)[:max_commands]
    return depth, pixels, dict(covered_pixels=int(covered.sum()), visible_commands=int(np.count_nonzero(pixels)),
                               foreign_pixels=int((covered & ~own).sum()))
