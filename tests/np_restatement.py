"""Independent numpy/float32 restatement of the cull predicates.

Written directly from the GLSL (shaders/entity_cull.comp, meshlet_cull.comp,
depth_reduce.comp in the reference repo), vectorised over all invocations, to
cross-check the C oracle (oracle/orbit_oracle.c): two restatements by different
means must agree bit-for-bit on visibility.  Every arithmetic step is a single
float32 numpy ufunc (no einsum/dot), so there is no contraction or
reassociation.  The entity stage's record scan is restated with repeat /
cumsum over whole arrays, the meshlet stage's words with plain python loops
(small cases only).
"""
import numpy as np

from orbit_amd import layouts as L

F = np.float32
S = 32

_C = np.array([float.fromhex(h) for h in (
    "0x1.715476p+0", "-0x1.71547p-1", "0x1.ec708p-2", "-0x1.715a68p-2", "0x1.2782e6p-2", "-0x1.eac694p-3",
    "0x1.a265fcp-3", "-0x1.865ffcp-3", "0x1.80ab18p-3", "-0x1.cebep-4")], dtype=np.float32)


def log2c(x):
    """The canonical software log2, vectorised."""
    x = np.asarray(x, dtype=np.float32).copy()
    out = np.empty_like(x)
    b = x.view(np.uint32)
    absb = b & np.uint32(0x7FFFFFFF)
    nan = absb > np.uint32(0x7F800000)
    zero = absb == 0
    neg = (b & np.uint32(0x80000000)) != 0
    inf = b == np.uint32(0x7F800000)
    sub = (b < np.uint32(0x00800000)) & ~zero & ~neg
    xs = np.where(sub, x * F(16777216.0), x).astype(np.float32)
    bs = xs.view(np.uint32)
    e = (bs >> np.uint32(23)).astype(np.int32) - 127 + np.where(sub, -24, 0)
    m = ((bs & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(np.float32)
    big = m > F(1.41421354)
    m = np.where(big, m * F(0.5), m).astype(np.float32)
    e = e + big
    f = (m - F(1.0)).astype(np.float32)
    p = np.full_like(f, _C[9])
    for i in range(8, -1, -1):
        p = (p * f).astype(np.float32)
        p = (p + _C[i]).astype(np.float32)
    r = (p * f).astype(np.float32)
    out[:] = (r + e.astype(np.float32)).astype(np.float32)
    out[zero] = -np.inf
    out[neg & ~zero] = np.nan
    out[inf] = np.inf
    out[nan] = x[nan]
    return out


def gmax(x, y):
    return np.where(x < y, y, x).astype(np.float32)


def gmin(x, y):
    return np.where(y < x, y, x).astype(np.float32)


def dot2(ax, ay, bx, by, contract=False):
    """`contract` (here and below): the oracle's arith_profile(1) — Dot / matrix products as fma chains in component order."""
    if contract:
        return fma32(ay, by, (ax * bx).astype(np.float32))
    return ((ax * bx).astype(np.float32) + (ay * by).astype(np.float32)).astype(np.float32)


def dot3(ax, ay, az, bx, by, bz, contract=False):
    if contract:
        return fma32(az, bz, fma32(ay, by, (ax * bx).astype(np.float32)))
    return ((ax * bx + ay * by).astype(np.float32) + (az * bz).astype(np.float32)).astype(np.float32)


def mat_vec(m, v0, v1, v2, v3, contract=False):
    """GLSL mat4 * vec4 for batched column-major m[..., 16] -> 4 arrays."""
    out = []
    for r in range(4):
        if contract:
            t = fma32(m[..., 4 + r], v1, (m[..., 0 + r] * v0).astype(np.float32))
            out.append(fma32(m[..., 12 + r], v3, fma32(m[..., 8 + r], v2, t)))
            continue
        t = (m[..., 0 + r] * v0 + m[..., 4 + r] * v1).astype(np.float32)
        t = (t + (m[..., 8 + r] * v2).astype(np.float32)).astype(np.float32)
        t = (t + (m[..., 12 + r] * v3).astype(np.float32)).astype(np.float32)
        out.append(t)
    return out


def mat_mul(a, b, contract=False):
    """a[16] (single) x b[n,16] -> [n,16], column-major."""
    a = np.broadcast_to(np.asarray(a, dtype=np.float32), b.shape)
    out = np.empty_like(b)
    for c in range(4):
        col = mat_vec(a, b[..., 4 * c + 0], b[..., 4 * c + 1], b[..., 4 * c + 2], b[..., 4 * c + 3], contract)
        for r in range(4):
            out[..., 4 * c + r] = col[r]
    return out


def fma32(a, b, c):
    """fma(a, b, c) rounded once to binary32 (what fmaf / v_fma_f32 compute): the product is exact in binary64, the
    sum is rounded to 53 bits and then to 24 — the second rounding is repaired where the 53-bit sum sits exactly half
    way between two binary32 values (TwoSum gives the sign of what the first rounding dropped)."""
    a, b, c = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in np.broadcast_arrays(a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    half = (np.ascontiguousarray(s).view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
    fix = half & (err != 0) & np.isfinite(s) & (np.abs(s) >= 2.0 ** -126)
    if np.any(fix):
        r64 = r.astype(np.float64)
        down = np.where(r64 > s, np.nextafter(r, np.float32(-np.inf)), r)
        up = np.where(r64 > s, r, np.nextafter(r, np.float32(np.inf)))
        r = np.where(fix, np.where(err > 0, up, down), r)
    return r.astype(np.float32)


RCP127 = np.frombuffer(np.array([0x3C010204], np.uint32).tobytes(), np.float32)[0]  # the compiled shaders' 1/127


def transform_sphere(m, sph, contract=False):
    one = np.ones(len(sph), dtype=np.float32)
    p = mat_vec(m, sph[:, 0], sph[:, 1], sph[:, 2], one, contract)
    with np.errstate(all="ignore"):
        x, y, z = (p[0] / p[3]).astype(F), (p[1] / p[3]).astype(F), (p[2] / p[3]).astype(F)
    dx = dot3(m[:, 0], m[:, 1], m[:, 2], m[:, 0], m[:, 1], m[:, 2], contract)
    dy = dot3(m[:, 4], m[:, 5], m[:, 6], m[:, 4], m[:, 5], m[:, 6], contract)
    dz = dot3(m[:, 8], m[:, 9], m[:, 10], m[:, 8], m[:, 9], m[:, 10], contract)
    scale = np.sqrt(gmax(dx, gmax(dy, dz)), dtype=np.float32)
    return x, y, z, (sph[:, 3] * scale).astype(np.float32), scale


def plane_test(ci, x, y, z, r, contract=False):
    vis = np.ones(len(x), dtype=bool)
    for i in range(int(ci["cull_plane_count"])):
        pl = ci["cull_planes"][i]
        d = (dot3(pl[0], pl[1], pl[2], x, y, z, contract) + pl[3]).astype(np.float32)
        vis &= d > -r
    return vis


def f2i_clamp(f, hi):
    f = np.asarray(f, dtype=np.float32)
    out = np.zeros(f.shape, dtype=np.int64)
    ok = f >= 0
    big = ok & (f > np.float32(hi))
    mid = ok & ~big
    out[big] = hi
    out[mid] = f[mid].astype(np.int64)
    return out


def pyramid_levels(w0, h0):
    mips = max(1, int(np.floor(np.log2(max(w0, h0)))) + 1)
    offs, ws, hs, off = [], [], [], 0
    for k in range(mips):
        w, h = max(w0 >> k, 1), max(h0 >> k, 1)
        offs.append(off)
        ws.append(w)
        hs.append(h)
        off += w * h
    return mips, np.array(offs), np.array(ws), np.array(hs), off


def footprint_min(img, w, h, u, v, detail=None):
    """img flat; w, h, u, v arrays (per sample).  `detail`, a dict, receives the unclamped texel coordinates fx, fy."""
    wf, hf = w.astype(np.float32), h.astype(np.float32)
    x = ((u * wf).astype(np.float32) - F(0.5)).astype(np.float32)
    y = ((v * hf).astype(np.float32) - F(0.5)).astype(np.float32)
    fx, fy = np.floor(x), np.floor(y)

    def cl(f, hi):
        f = np.asarray(f, dtype=np.float32)
        out = np.zeros(f.shape, dtype=np.int64)
        ok = f >= 0
        big = ok & (f > hi.astype(np.float32))
        mid = ok & ~big
        out[big] = hi[big]
        out[mid] = f[mid].astype(np.int64)
        return out
    x0, x1 = cl(fx, w - 1), cl((fx + F(1)).astype(F), w - 1)
    y0, y1 = cl(fy, h - 1), cl((fy + F(1)).astype(F), h - 1)
    if detail is not None:
        detail.update(fx=fx, fy=fy)
    return x0, x1, y0, y1


def hiz_sample(pyr, w0, h0, u, v, lod, detail=None):
    """`detail`, a dict, receives the intermediates (tests/hiz_edges.py takes its census from them): mips, the level and
    its size, the unclamped and the clamped footprint, the four texels' indices in the packed chain, the result."""
    mips, offs, ws, hs, _ = pyramid_levels(w0, h0)
    with np.errstate(all="ignore"):
        lf = (np.ceil((lod + F(0.5)).astype(F)) - F(1.0)).astype(np.float32)
    level = f2i_clamp(lf, mips - 1)
    w, h, off = ws[level], hs[level], offs[level]
    x0, x1, y0, y1 = footprint_min(pyr, w, h, u, v, detail)
    a, b = pyr[off + y0 * w + x0], pyr[off + y0 * w + x1]
    c, d = pyr[off + y1 * w + x0], pyr[off + y1 * w + x1]
    sampled = gmin(gmin(a, b), gmin(c, d))
    if detail is not None:
        detail.update(mips=mips, level=level, w=w, h=h, x0=x0, x1=x1, y0=y0, y1=y1, sampled=sampled,
                      texels=np.stack([off + y0 * w + x0, off + y0 * w + x1, off + y1 * w + x0, off + y1 * w + x1]))
    return sampled


def occlusion_test(ci, x, y, z, r, pyr, pw, ph, radius, scale, detail=None, contract=False):
    """Returns (visible, z') — z' is the possibly flipped z (persists).  Operation by operation as the reference's
    compiled shaders hold it (oracle/orbit_oracle.c occlusion_test): radius = model-space radius, r = radius * scale.
    `detail`, a dict, receives cullable (and where it is decided by equality), u, v, lod, closest and hiz_sample's
    intermediates, per row."""
    n = len(x)
    with np.errstate(all="ignore"):
        if int(ci["projection_type"]) == 0:
            z = (-z).astype(np.float32)
            zn = F(ci["z_near"])
            near = fma32(radius, scale, zn)
            cullable = z >= near
            if detail is not None:
                detail["cullable_tie"] = z == near
            p00, p11 = F(ci["p00_or_width_recipx2"]), F(ci["p11_or_height_recipx2"])

            def bounds(c0, c1):
                # cx = -C.xz ; vx = (sqrt(dot(cx,cx) - r*r), r)
                vx = np.sqrt(fma32(-r, r, dot2(c0, c1, c0, c1, contract)), dtype=F)
                vy = r
                mn_x, mn_y = dot2(vx, (-vy).astype(F), c0, c1, contract), dot2(vy, vx, c0, c1, contract)
                mx_x, mx_y = dot2(vx, vy, c0, c1, contract), dot2((-vy).astype(F), vx, c0, c1, contract)
                return mn_x, mn_y, mx_x, mx_y
            minx_x, minx_y, maxx_x, maxx_y = bounds((-x).astype(F), (-z).astype(F))
            miny_x, miny_y, maxy_x, maxy_y = bounds((-y).astype(F), (-z).astype(F))
            a0 = ((minx_x / minx_y).astype(F) * p00).astype(F)
            a1 = ((miny_x / miny_y).astype(F) * p11).astype(F)
            a2 = ((maxx_x / maxx_y).astype(F) * p00).astype(F)
            a3 = ((maxy_x / maxy_y).astype(F) * p11).astype(F)
            u0 = fma32(a0, F(0.5), F(0.5))
            v0 = fma32(a3, F(-0.5), F(0.5))
            u1 = fma32(a2, F(0.5), F(0.5))
            v1 = fma32(a1, F(-0.5), F(0.5))
            closest = (zn / fma32(-radius, scale, z)).astype(F)
        else:
            sr = F(ci["p00_or_width_recipx2"])
            cx, cy = (x * sr).astype(F), (y * sr).astype(F)
            bs = (sr * r).astype(F)
            b0, b1 = fma32(bs, F(-1.0), cx), fma32(bs, F(-1.0), cy)
            b2, b3 = fma32(bs, F(1.0), cx), fma32(bs, F(1.0), cy)
            cl = lambda t: gmin(gmax(t, F(-1.0)), F(1.0))
            u0 = fma32(cl(b0), F(0.5), F(0.5))
            v0 = fma32(cl(b1), F(-0.5), F(0.5))
            u1 = fma32(cl(b2), F(0.5), F(0.5))
            v1 = fma32(cl(b3), F(-0.5), F(0.5))
            cullable = np.ones(n, dtype=bool)
            if detail is not None:
                detail["cullable_tie"] = np.zeros(n, dtype=bool)
            rr = F(1.0) / (F(ci["z_far"]) - F(ci["z_near"]))
            closest = (rr * (fma32(radius, scale, z) + F(ci["z_far"])).astype(F)).astype(F)
        width = ((u1 - u0).astype(F) * F(pw)).astype(F)
        height = ((v1 - v0).astype(F) * F(ph)).astype(F)
        u = ((u0 + u1).astype(F) * F(0.5)).astype(F)
        v = ((v0 + v1).astype(F) * F(0.5)).astype(F)
        lod = log2c(gmax(width, height))
        sampled = hiz_sample(pyr, pw, ph, u, v, lod, detail)
        vis = np.where(cullable, closest >= sampled, True)
    if detail is not None:
        detail.update(cullable=cullable, u=u, v=v, lod=lod, closest=closest, visible=vis)
    return vis, z


def f2u_sat(f):
    f = np.asarray(f, dtype=np.float32)
    out = np.zeros(f.shape, dtype=np.uint64)
    pos = f > 0
    big = pos & (f >= F(4294967296.0))
    mid = pos & ~big
    out[big] = 0xFFFFFFFF
    out[mid] = f[mid].astype(np.uint64)
    return out


def entity_cull(ci, scene_draws, count, entity_draw_count, mesh_infos, entities, vis_words, pyr=None, pyr_size=(0, 0),
                detail=None, S=32, contract=False):
    """Returns (visible[g], should_draw[g], records list, new entity words or None).  `detail`, a dict, receives
    occlusion_test's intermediates of pass 2 and `reached`, the rows that got as far as that test, and per draw the
    `mesh_lod` it picks and the `meshlets` and `records` it emits.  S: MESHLET_DISPATCH_SIZE of the records (pass 0);
    contract: the oracle's arith_profile(1)."""
    end = min(count, (entity_draw_count + 255) // 256 * 256)
    draws = scene_draws[:end]
    g = np.arange(end)
    mi = mesh_infos[draws["mesh_index"]]
    en = entities[draws["entity_index"]]
    op = int(ci["occlusion_pass"])
    meshlet_occ = int(ci["meshlet_visibility_buffer"]) != L.NONE
    vib = np.ones(end, dtype=bool)
    if op in (1, 2):
        vib = ((vis_words[g // 32] >> (g % 32).astype(np.uint32)) & 1).astype(bool)
    visible = vib.copy() if op == 1 else np.ones(end, dtype=bool)
    mv = mat_mul(ci["view_matrix"], en["model_matrix"], contract)
    x, y, z, r, scale = transform_sphere(mv, mi["bounding_sphere"], contract)
    visible &= np.where(visible, plane_test(ci, x, y, z, r, contract), False)
    if op == 2:
        ov, zf = occlusion_test(ci, x, y, z, r, pyr, *pyr_size, mi["bounding_sphere"][:, 3].astype(F), scale, detail, contract)
        if detail is not None:
            detail["reached"] = visible.copy()
        z = np.where(visible, zf, z).astype(np.float32) if int(ci["projection_type"]) == 0 else z
        visible = np.where(visible, ov, False)
    should = visible.copy()
    if op == 2:
        should = visible & (~vib | meshlet_occ)
    t = ci["lod_target_pos_view_space"]
    ex, ey, ez = (t[0] - x).astype(F), (t[1] - y).astype(F), (t[2] - z).astype(F)
    with np.errstate(all="ignore"):
        dist = (np.sqrt(dot3(ex, ey, ez, ex, ey, ez, contract), dtype=F) - r).astype(F)
        lf = (log2c((gmax(dist, F(0.0)) / F(ci["lod_base"])).astype(F)) / log2c(np.array([ci["lod_step"]], F))).astype(F)
        lod = f2u_sat(gmax((lf + F(1.0)).astype(F), F(0.0)))
    lod = np.minimum(np.maximum(lod, int(ci["min_mesh_lod"])), int(ci["max_mesh_lod"]))
    lod = np.minimum(lod, (mi["lod_count"].astype(np.uint64) - 1) & 0xFFFFFFFF)
    lod = np.minimum(lod, 7).astype(np.int64)
    if detail is not None:  # per draw: the LOD it would pick, the meshlets and records it emits
        cnt = np.where(should, mi["mesh_lods"][g, lod, 1].astype(np.int64), 0) if end else np.zeros(0, np.int64)
        detail.update(mesh_lod=lod, meshlets=cnt, records=(cnt + S - 1) // S)
    # record j of a draw: every record before it is full, so its word offset has advanced by j (c // S == 1 each)
    idx = np.nonzero(should)[0]
    off, cnt = (mi["mesh_lods"][idx, lod[idx], k].astype(np.int64) for k in (0, 1))
    per = (cnt + S - 1) // S
    own = np.repeat(np.arange(len(idx)), per)
    j = np.arange(int(per.sum())) - np.repeat(np.cumsum(per) - per, per)
    records = np.stack([draws["entity_index"][idx][own].astype(np.int64), off[own] + S * j,
                        np.minimum(cnt[own] - S * j, S), draws["visibility_offset"][idx][own].astype(np.int64) + j],
                       axis=1) & 0xFFFFFFFF
    new_words = None
    if op == 2:
        new_words = vis_words.copy()
        bits = np.zeros((end + 31) // 32 * 32, dtype=np.uint64)
        bits[:end] = visible
        new_words[:len(bits) // 32] = (bits.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    return visible, should, np.ascontiguousarray(records.astype(np.uint32)).view(L.MESHLET_DISPATCH).reshape(-1), new_words


def meshlet_cull(ci, records, meshlets, entities, materials, mvis, pyr=None, pyr_size=(0, 0), detail=None):
    """Returns (commands, new meshlet visibility words or None).  `detail`: as for entity_cull."""
    op = int(ci["occlusion_pass"])
    meshlet_occ = int(ci["meshlet_visibility_buffer"]) != L.NONE
    nrec = len(records)
    lane = np.tile(np.arange(S), nrec)
    rid = np.repeat(np.arange(nrec), S)
    active = lane < records["meshlet_count"][rid]
    rid, lane = rid[active], lane[active]
    rec = records[rid]
    idx = rec["meshlet_offset"].astype(np.int64) + lane
    m = meshlets[idx]
    mv = mat_mul(ci["view_matrix"], entities["model_matrix"][rec["entity_index"]])
    x, y, z, r, scale = transform_sphere(mv, m["bounding_sphere"])
    ax = (m["cone_axis"].astype(np.int32).astype(np.float32) * RCP127).astype(F)
    axis = mat_vec(mv, ax[:, 0], ax[:, 1], ax[:, 2], np.zeros(len(ax), F))
    cutoff = (m["cone_cutoff"].astype(np.int32).astype(np.float32) * RCP127).astype(F)
    alpha = materials["alpha_mode"][m["material_index"]]
    rw = op in (1, 2) and meshlet_occ
    vib = np.ones(len(idx), dtype=bool)
    if rw:
        vib = ((mvis[rec["visibility_offset"] + lane // 32] >> (lane % 32).astype(np.uint32)) & 1).astype(bool)
    visible = vib.copy() if op == 1 else np.ones(len(idx), dtype=bool)
    visible &= plane_test(ci, x, y, z, r)
    with np.errstate(all="ignore"):
        if int(ci["projection_type"]) == 1:
            camx, camy, camz = (x - F(0)).astype(F), (y - F(0)).astype(F), (z - F(-1.0)).astype(F)
        else:
            camx = camy = camz = np.zeros(len(x), F)
        dx, dy, dz = (x - camx).astype(F), (y - camy).astype(F), (z - camz).astype(F)
        lhs = dot3(dx, dy, dz, axis[0], axis[1], axis[2])
        rhs = fma32(cutoff, np.sqrt(dot3(dx, dy, dz, dx, dy, dz), dtype=F), r)
        visible &= ~(lhs >= rhs)
    if meshlet_occ and op == 2:
        ov, _ = occlusion_test(ci, x, y, z, r, pyr, *pyr_size, m["bounding_sphere"][:, 3].astype(F), scale, detail)
        if detail is not None:
            detail["reached"] = visible.copy()
        visible = np.where(visible, ov, False)
    shl = lambda a: np.where(a < 32, np.uint64(1) << a.astype(np.uint64), 0).astype(np.uint64)
    should = visible & ((shl(alpha) & np.uint64(int(ci["alpha_mode_flag"]))) != 0)
    if op == 2 and meshlet_occ:
        skip = (shl(alpha) & np.uint64(int(ci["noskip_alphamode"]))) != 0
        should = np.where(~skip, visible & ~vib, should)
    cmds = np.zeros(int(should.sum()), dtype=L.MESHLET_DRAW_COMMAND)
    ms = m[should]
    cmds["cmd_index_count"] = ms["triangle_count"].astype(np.uint32) * 3
    cmds["cmd_instance_count"] = 1
    cmds["cmd_first_index"] = (ms["data_offset"] + ms["vertex_count"].astype(np.uint32)) * np.uint32(4)
    cmds["cmd_vertex_offset"] = ms["data_offset"].view(np.int32)
    cmds["cmd_first_instance"] = rec["entity_index"][should]
    cmds["meshlet_vertex_offset"] = ms["vertex_offset"]
    cmds["meshlet_index"] = idx[should].astype(np.uint32)
    if detail is not None:  # per active lane: its record, its lane, its verdict
        detail.update(record=rid, lane=lane, should_draw=should)
    new = None
    if op == 2 and meshlet_occ:
        # every word an active lane lies in is REPLACED by the visible bits of its lanes
        new = mvis.copy()
        w = rec["visibility_offset"].astype(np.int64) + lane // 32
        acc = np.zeros(len(new), dtype=np.uint32)
        np.bitwise_or.at(acc, w, visible.astype(np.uint32) << (lane % 32).astype(np.uint32))
        touched = np.unique(w)
        new[touched] = acc[touched]
    return cmds, new


def depth_reduce(depth, sw, sh):
    from math import floor, log2

    def npot(v):
        p = 1
        while p < v:
            p <<= 1
        return p
    w0, h0 = max(npot(sw) // 2, 1), max(npot(sh) // 2, 1)
    mips, offs, ws, hs, total = pyramid_levels(w0, h0)
    pyr = np.zeros(total, dtype=np.float32)
    src, srcw, srch = np.ascontiguousarray(depth, np.float32).reshape(-1), sw, sh
    for k in range(mips):
        dw, dh = int(ws[k]), int(hs[k])
        ys, xs = np.mgrid[0:dh, 0:dw]
        u = ((xs.astype(F) + F(0.5)) / F(dw)).astype(F).reshape(-1)
        v = ((ys.astype(F) + F(0.5)) / F(dh)).astype(F).reshape(-1)
        W = np.full(u.shape, srcw)
        H = np.full(u.shape, srch)
        x0, x1, y0, y1 = footprint_min(src, W, H, u, v)
        a, b = src[y0 * srcw + x0], src[y0 * srcw + x1]
        c, d = src[y1 * srcw + x0], src[y1 * srcw + x1]
        lvl = gmin(gmin(a, b), gmin(c, d))
        pyr[offs[k]:offs[k] + dw * dh] = lvl
        src, srcw, srch = lvl, dw, dh
    return pyr, (w0, h0, mips)


# ----------------------------------------------------------------------------- light clusters (light_culling.comp)
def _field(info, name):
    return np.asarray(info).reshape(-1)[0][name]


def cluster_aabb(info, bounds, cluster_index):
    """compute_cluster_volume (light_culling.comp:62-90) of every cluster in `cluster_index` -> (mn[n, 3], mx[n, 3]).
    screen_to_view and line_intersection_to_z_plane as written (eye = 0, normal = (0, 0, -1), dot products left to
    right); min / max are the GLSL's (y < x ? y : x) forms the oracle documents."""
    cx, cy = (int(v) for v in _field(info, "cluster_count")[:2])
    tile = int(_field(info, "tile_size_px"))
    sw, sh = (F(int(v)) for v in _field(info, "screen_size"))
    s2v = np.asarray(_field(info, "screen_to_view_matrix"), F)
    z_near = F(_field(info, "z_near"))
    idx = np.asarray(cluster_index, np.int64).reshape(-1)
    z = idx // (cx * cy)
    rem = idx - z * cx * cy
    y = rem // cx
    x = rem - y * cx
    with np.errstate(all="ignore"):
        min_x, min_y = (x * tile).astype(F), (y * tile).astype(F)  # cluster_id.xy * tile_size_px, :67
        max_x, max_y = gmin((min_x + F(tile)).astype(F), sw), gmin((min_y + F(tile)).astype(F), sh)  # :68

        def screen_to_view(sx, sy):  # :34-48
            tx, ty = (sx / sw).astype(F), (sy / sh).astype(F)
            c0 = (tx * F(2.0) - F(1.0)).astype(F)
            c1 = ((F(1.0) - ty).astype(F) * F(2.0) - F(1.0)).astype(F)
            one = np.ones_like(c0)
            v = mat_vec(s2v, c0, c1, one, one)
            return [(v[i] / v[3]).astype(F) for i in range(3)]

        def line_z(b, zd):  # :50-60 with a = 0
            ab = [(t - F(0.0)).astype(F) for t in b]
            dna = F(F(0.0) * F(0.0) + F(0.0) * F(0.0)) + F(-1.0) * F(0.0)
            dnab = (((F(0.0) * ab[0]).astype(F) + (F(0.0) * ab[1]).astype(F)).astype(F) + (F(-1.0) * ab[2]).astype(F)).astype(F)
            t = ((zd - dna).astype(F) / dnab).astype(F)
            return [(F(0.0) + (t * a).astype(F)).astype(F) for a in ab]

        lo, hi = screen_to_view(min_x, min_y), screen_to_view(max_x, max_y)
        b = np.ascontiguousarray(bounds, np.uint32)[idx]
        min_depth = (F(1.0) - b[:, 0].view(F)).astype(F)
        max_depth = b[:, 1].view(F)
        near, far = (z_near / max_depth).astype(F), (z_near / min_depth).astype(F)
        p = [line_z(lo, near), line_z(lo, far), line_z(hi, near), line_z(hi, far)]
        mn = np.stack([gmin(gmin(p[0][i], p[1][i]), gmin(p[2][i], p[3][i])) for i in range(3)], axis=1)
        mx = np.stack([gmax(gmax(p[0][i], p[1][i]), gmax(p[2][i], p[3][i])) for i in range(3)], axis=1)
    return mn, mx


def light_view_centres(info, lights):
    """world_to_view_matrix * vec4(position, 1.0) of every light (:110) -> [n, 3]."""
    pos = np.asarray(lights["position"], F)
    with np.errstate(all="ignore"):
        c = mat_vec(np.asarray(_field(info, "world_to_view_matrix"), F), pos[:, 0], pos[:, 1], pos[:, 2],
                    np.ones(len(pos), F))
    return np.stack(c[:3], axis=1)


def lights_in_clusters(mn, mx, centres, radius, point):
    """is_light_in_cluster (:108-119) for every (cluster, light) pair -> bool[clusters, lights]: a non-point light is in
    every cluster; a point light by aabb_sphere_test, whose sum the binary compiles to sqr_dist = fma(d, d, sqr_dist)."""
    with np.errstate(all="ignore"):
        sq = np.zeros((len(mn), len(centres)), F)
        for i in range(3):
            v = centres[None, :, i]
            for inside, d in ((v < mn[:, i:i + 1], mn[:, i:i + 1] - v), (v > mx[:, i:i + 1], v - mx[:, i:i + 1])):
                if inside.any():
                    d = np.broadcast_to(d.astype(F), sq.shape)[inside]
                    sq[inside] = fma32(d, d, sq[inside])
        r = np.asarray(radius, F)
        return ~np.asarray(point, bool)[None, :] | (sq <= (r * r).astype(F)[None, :])


def cluster_assign(info, unique, bounds, lights, light_index_capacity, total_clusters, max_lights_per_cluster=256):
    """light_culling.comp:121-151 for the compacted list `unique`, ranges allocated in list order (the oracle's
    canonical order of the atomicAdd): the first min(count, 256) hits of every cluster in light order.  Returns
    (index buffer with its light_count header, (offset, count) image, the UNCAPPED count of every listed cluster,
    indices dropped past light_index_capacity)."""
    unique = np.asarray(unique, np.uint8)
    n = int(unique[12:16].view(np.uint32)[0])
    act = unique[16:16 + 4 * n].view(np.uint32)
    nl = int(_field(info, "global_light_count"))
    lights = np.asarray(lights)[:nl]
    centres = light_view_centres(info, lights)
    point = lights["light_type"] == L.LIGHT_TYPE_POINT
    hits = np.zeros((n, nl), bool)
    step = max(1, (1 << 21) // max(nl, 1))
    for c0 in range(0, n, step):
        mn, mx = cluster_aabb(info, bounds, act[c0:c0 + step])
        hits[c0:c0 + step] = lights_in_clusters(mn, mx, centres, lights["outer_radius"], point)
    count = hits.sum(axis=1).astype(np.int64)
    capped = np.minimum(count, max_lights_per_cluster)
    kept = hits & (np.cumsum(hits, axis=1) <= max_lights_per_cluster)
    indices = np.nonzero(kept)[1].astype(np.uint32)  # row-major: cluster by cluster in list order, ascending lights
    offsets = np.cumsum(capped) - capped
    out = np.zeros(4 + 4 * light_index_capacity, np.uint8)
    out[:4] = np.array([int(capped.sum())], np.uint32).view(np.uint8)
    kept_n = min(len(indices), light_index_capacity)
    out[4:4 + 4 * kept_n] = indices[:kept_n].view(np.uint8)
    img = np.zeros((total_clusters, 2), np.uint32)
    img[act, 0], img[act, 1] = offsets, capped
    return out, img, count, len(indices) - kept_n
