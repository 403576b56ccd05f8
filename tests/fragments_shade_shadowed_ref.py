"""orbit_fragments_shade_shadowed restated in numpy float32 from the rules H1-H10 (and L1-L9) of include/orbit_abi_ext.h —
an independent restatement that shares nothing with orbit_amd/csrc/shadow_common.h: its own sine and cosine, written from
H6's text, its own offset table, the walk position by position over all pixels at once, every float32 operation numpy's
(each rounded on its own, no fused multiply-add).  L1 / L2 come from fragments_shade_ref.classify.  `shadow64` is the GLSL
in float64 with the true sin / cos: what the accuracy figure of tools/count_fragments_shade_shadowed.py is measured
against."""
import numpy as np

import fragments_shade_ref as base
from orbit_amd import _lib
from orbit_amd import layouts as L

F = np.float32
NONE = 0xFFFFFFFF
PI = base.PI
SHADOW_STATS = ("shadowed_pixels", "no_cascade_pixels", "early_out_pixels", "shadow_evaluations")

# poisson_offsets[0..31], forward.frag:14-79
POISSON = np.array([
    (0.0617981, 0.07294159), (0.6470215, 0.7474022), (-0.5987766, -0.7512833), (-0.693034, 0.6913887), (0.6987045, -0.6843052),
    (-0.9402866, 0.04474335), (0.8934509, 0.07369385), (0.1592735, -0.9686295), (-0.05664673, 0.995282), (-0.1203411, -0.1301079),
    (0.1741608, -0.1682285), (-0.09369049, 0.3196758), (0.185363, 0.3213367), (-0.1493771, -0.3147511), (0.4452095, 0.2580113),
    (-0.1080467, -0.5329178), (0.1604507, 0.5460774), (-0.4037193, -0.2611179), (0.5947998, -0.2146744), (0.3276062, 0.9244621),
    (-0.6518704, -0.2503952), (-0.3580975, 0.2806469), (0.8587891, 0.4838005), (-0.1596546, -0.8791054), (-0.3096867, 0.5588146),
    (-0.5128918, 0.1448544), (0.8581337, -0.424046), (0.1562584, -0.5610626), (-0.7647934, 0.2709858), (-0.3090832, 0.9020988),
    (0.3935608, 0.4609676), (0.3929337, -0.5010948)], F)


def fract(a):
    return a - np.floor(a)


def theta_of(xs, ys):
    """H6's angle of the pixels (xs, ys)"""
    sx, sy = xs.astype(F) + F(0.5), ys.astype(F) + F(0.5)
    ign = fract(F(52.9829189) * fract(sx * F(0.06711056) + sy * F(0.00583715)))
    return (ign * F(2)) * PI


def sincos(theta):
    """H6's sinc and cosc"""
    theta = np.asarray(theta, F)
    k = (theta * F(0.636619772) + F(0.5)).astype(np.int32)
    kf = k.astype(F)
    r = (theta - kf * F(1.5703125)) - kf * F(4.83826794897e-4)
    w = r * r
    sin_r = ((((F(-1.9515295891e-4) * w + F(8.3321608736e-3)) * w) + F(-1.6666654611e-1)) * w) * r + r
    cos_r = ((((F(2.443315711809948e-5) * w + F(-1.388731625493765e-3)) * w) + F(4.166664568298827e-2)) * w) * w + (F(1) - F(0.5) * w)
    q = k & 3
    s = np.choose(q, [sin_r, cos_r, -sin_r, -cos_r]).astype(F)
    c = np.choose(q, [cos_r, -sin_r, -cos_r, sin_r]).astype(F)
    return s, c


def project(M, x, y, z, w):
    """R2's left-to-right sums: M (n, 16) column-major times (x, y, z, w) -> (n, 4)"""
    return np.stack([((M[:, r] * x + M[:, 4 + r] * y) + M[:, 8 + r] * z) + M[:, 12 + r] * w for r in range(4)], axis=1).astype(F)


def texel(f, res):
    """clamp((int)f, 0, res - 1) of floored floats, saturating, NaN -> 0"""
    return np.where(f > 0, np.where(f >= F(res), res - 1, np.where(np.isfinite(f), f, 0)), 0).astype(np.int64)


def evaluate(rows, wp4, N, direction, inner_radius, xs, ys, maps, map_count, res, blocker_search_radius, normal_bias_scale, oriented_bias):
    """H2-H8 of one shadowed light per entry -> (shadow float32, cascade, stale, early_out, lit taps or -1, blockers or -1)"""
    n = len(rows)
    shadow, cascade = np.ones(n, F), np.full(n, 4, np.int64)
    stale, early, lit_out, blockers = np.zeros(n, bool), np.zeros(n, bool), np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    Ms = rows["light_projection_matrices"]
    for i in (3, 2, 1, 0):  # the first inside wins: later ones are overwritten
        c = project(Ms[:, i], wp4[:, 0], wp4[:, 1], wp4[:, 2], wp4[:, 3])
        q = c / c[:, 3:4]
        inside = (q[:, 0] >= -1) & (q[:, 1] >= -1) & (q[:, 2] >= 0) & (q[:, 3] >= 0) & (q <= 1).all(axis=1)
        cascade[inside] = i
    have = np.flatnonzero(cascade < 4)
    cas = cascade[have]
    which = rows["shadow_map_indices"][have, cas].astype(np.int64)
    bad = which >= map_count
    stale[have[bad]] = True
    have, cas, which = have[~bad], cas[~bad], which[~bad]
    if not len(have):
        return shadow, cascade, stale, early, lit_out, blockers
    resf = F(res)
    tx = F(1) / resf
    Nn, d, wp = N[have], direction[have], wp4[have, :3]
    ndl = base.dot(Nn, d)
    nos = base.gclamp(F(1) - ndl, F(0), F(1))
    scale = (tx * F(normal_bias_scale)) * nos
    ob = np.where(ndl > 0, -F(oriented_bias), F(oriented_bias)).astype(F)
    sp = (wp + scale[:, None] * Nn) + ob[:, None] * d
    c = project(Ms[have, cas], sp[:, 0], sp[:, 1], sp[:, 2], F(1))
    z = c[:, 2] / c[:, 3]
    u = (c[:, 0] / c[:, 3] + F(1)) * F(0.5)
    v = ((c[:, 1] / c[:, 3]) * F(-1) + F(1)) * F(0.5)
    inv_ws = F(1) / rows["shadow_map_world_sizes"][have, cas]
    light_uv = inner_radius[have] * inv_ws
    s, cs = sincos(theta_of(xs[have], ys[have]))
    origin = which * res * res
    rad = F(blocker_search_radius) * inv_ws
    avg, count = np.zeros(len(have), F), np.zeros(len(have), np.int64)
    for ox, oy in POISSON[:12]:
        rx, ry = cs * ox + (-s) * oy, s * ox + cs * oy
        su, sv = u + (rx * rad) * inv_ws, v + (ry * rad) * inv_ws
        t = maps[origin + texel(np.floor(sv * resf), res) * res + texel(np.floor(su * resf), res)]
        blocked = t > z
        avg = np.where(blocked, avg + (F(1) - t), avg).astype(F)
        count += blocked
    out = (count == 0) | (count == 12)
    early[have], blockers[have] = out, count
    shadow[have] = np.where(count == 0, F(1), F(0))
    avg = avg / count.astype(F)
    pen = (((F(1) - z) - avg) / avg) * light_uv
    fr = base.gmax(pen * inv_ws, tx)
    lit = np.zeros(len(have), np.int64)
    for ox, oy in POISSON:
        rx, ry = cs * ox + (-s) * oy, s * ox + cs * oy
        fx, fy = np.floor((u + rx * fr) * resf - F(0.5)), np.floor((v + ry * fr) * resf - F(0.5))
        x0, x1, y0, y1 = texel(fx, res), texel(fx + F(1), res), texel(fy, res) * res, texel(fy + F(1), res) * res
        for at in (y0 + x0, y0 + x1, y1 + x0, y1 + x1):
            lit += z >= maps[origin + at]
    filtered = have[~out]
    shadow[filtered] = lit[~out].astype(F) / F(128)
    lit_out[filtered] = lit[~out]
    return shadow, cascade, stale, early, lit_out, blockers


def light_terms(l, wp, N, V, albedo, metallic, r, cutoff):
    """L5 / L6 of point and directional lights `l` at the pixels -> the terms (n, 3)"""
    point = l["light_type"] == L.LIGHT_TYPE_POINT
    lc = l["color"] * l["intensity"][:, None]
    Ld = l["position"] - wp
    dist = np.sqrt(base.dot(Ld, Ld))
    Ld = Ld / dist[:, None]
    dist = base.gmax(dist, l["inner_radius"])
    d2 = dist * dist
    att = base.gmax(l["intensity"] / d2 - (cutoff * d2) / (l["outer_radius"] * l["outer_radius"]), F(0))
    Ld = np.where(point[:, None], Ld, l["direction"]).astype(F)
    att = np.where(point, att, F(1)).astype(F)
    H = base.normalize(V + Ld)
    ndv, ndl = base.gmax(base.dot(N, V), base.EPS), base.gmax(base.dot(N, Ld), base.EPS)
    ndh, hv = base.gmax(base.dot(N, H), F(0)), base.gmax(base.dot(H, V), F(0))
    a = r * r
    a2 = a * a
    den = (ndh * ndh) * (a2 - F(1)) + F(1)
    den = (PI * den) * den
    D = a2 / base.gmax(den, base.EPS)
    rr = r + F(1)
    k = (rr * rr) / F(8)
    G = (ndv / (ndv * (F(1) - k) + k)) * (ndl / (ndl * (F(1) - k) + k))
    f0 = F(0.04) * (F(1) - metallic)[:, None] + albedo * metallic[:, None]
    x = F(1) - hv
    p5 = ((x * x) * (x * x)) * x
    Fr = f0 + (F(1) - f0) * p5[:, None]
    spec = ((D * G)[:, None] * Fr) / ((F(4) * ndv) * ndl)[:, None]
    kD = (F(1) - Fr) * (F(1) - metallic)[:, None]
    return (((((kD * albedo) / PI) + spec) * (lc * att[:, None])) * ndl[:, None]).astype(F)


def shade(oracle, vis, world_pos, normal, material, materials, lights, image, index_buffer, cluster_count, tile_size_px, z_scale, z_bias,
          luminance_cutoff, z_near, view_pos, shadows, shadow_maps, shadow_resolution, blocker_search_radius, normal_bias_scale,
          oriented_bias, shadow_index_base=0, shadow_count=None, shadow_map_count=None, render_mode=0, clear=True, fill=0,
          material_count=None, light_count=None, index_capacity=None):
    """-> the dict of orbit_amd.raster.host_fragments_shade_shadowed (every optional output present), and `lit`: the lit
    taps and `blockers`: the blocker count of the first shadowed light per pixel (-1 where H8 / H7 did not run)"""
    vis = np.asarray(vis, np.uint64)
    h, w = vis.shape
    c = base.classify(oracle, vis, material, materials, lights, image, index_buffer, cluster_count, tile_size_px, z_scale, z_bias, z_near,
                      material_count, light_count, index_capacity)
    n, offset, indices = c["n"], c["offset"], c["indices"]
    mats = np.ascontiguousarray(materials).view(np.uint8).reshape(-1)
    mats = mats[:len(mats) // 80 * 80].view(L.MATERIAL)
    lts = np.ascontiguousarray(lights).view(np.uint8).reshape(-1)
    lts = lts[:len(lts) // 64 * 64].view(L.LIGHT)
    res = int(shadow_resolution)
    rows = np.zeros(0, L.SHADOW_DATA) if shadows is None else np.ascontiguousarray(shadows).view(np.uint8).reshape(-1)
    rows = rows if shadows is None else rows[:len(rows) // 288 * 288].view(L.SHADOW_DATA)
    maps = np.zeros(0, F) if shadow_maps is None else np.ascontiguousarray(shadow_maps, F).reshape(-1)
    shadow_count = len(rows) if shadow_count is None else shadow_count
    shadow_map_count = (len(maps) // (res * res) if res else 0) if shadow_map_count is None else shadow_map_count
    pix = np.flatnonzero(c["live"])
    ys, xs = np.divmod(pix, w)
    m = mats[np.asarray(material, np.uint32).reshape(-1)[pix]]
    textured = (m["texture_indices"] != NONE).any(axis=1)
    count = len(pix)
    unserved, degenerate, stale = np.zeros(count, bool), np.zeros(count, bool), np.zeros(count, bool)
    factor, cascade, lit_first = np.ones(count, F), np.full(count, NONE, np.uint32), np.full(count, -1, np.int64)
    blockers_first = np.full(count, -1, np.int64)
    evaluations = np.zeros(count, np.int64)
    no_cascade, early_out = np.zeros(count, bool), np.zeros(count, bool)
    n_p, off_p = n[pix], offset[pix]
    wp4 = np.asarray(world_pos, F).reshape(-1, 4)[pix]
    N = np.asarray(normal, F).reshape(-1, 3)[pix]
    with np.errstate(all="ignore"):
        albedo, metallic, r = m["base_color"][:, :3].astype(F), m["metallic_factor"].astype(F), m["roughness_factor"].astype(F)
        V = base.normalize(np.asarray(view_pos, F)[None, :] - wp4[:, :3])
        total = m["emissive_factor"].astype(F).copy()
        cutoff = F(luminance_cutoff)
        for i in range(int(n_p.max()) if count else 0):
            at = np.flatnonzero((n_p > i) & ~stale)
            l = lts[indices[off_p[at] + i]]
            kind = l["light_type"]
            shadowed = (kind == L.LIGHT_TYPE_DIRECTIONAL) & (l["shadow_data_index"] != NONE)
            row = (l["shadow_data_index"].astype(np.int64) - shadow_index_base) % (1 << 32)  # H1, u32 arithmetic
            bad = shadowed & (row >= shadow_count)
            stale[at[bad]] = True
            at, l, kind, shadowed, row = at[~bad], l[~bad], kind[~bad], shadowed[~bad], row[~bad]
            if render_mode == 8:
                continue
            unserved[at] |= kind == L.LIGHT_TYPE_SKY
            lit = (kind == L.LIGHT_TYPE_POINT) | (kind == L.LIGHT_TYPE_DIRECTIONAL)
            at, l, kind, shadowed, row = at[lit], l[lit], kind[lit], shadowed[lit], row[lit]
            if not len(at):
                continue
            term = light_terms(l, wp4[at, :3], N[at], V[at], albedo[at], metallic[at], r[at], cutoff)
            shadow = np.ones(len(at), F)
            sh = np.flatnonzero(shadowed)
            if len(sh):
                p = at[sh]
                s_, cas, bad, early, lit_taps, blocked = evaluate(rows[row[sh]], wp4[p], N[p], l["direction"][sh], l["inner_radius"][sh], xs[p], ys[p],
                                                         maps, shadow_map_count, res, blocker_search_radius, normal_bias_scale,
                                                         oriented_bias)
                stale[p[bad]] = True
                good = ~bad
                first = good & (evaluations[p] == 0)
                factor[p[first]], cascade[p[first]], lit_first[p[first]] = s_[first], cas[first], lit_taps[first]
                blockers_first[p[first]] = blocked[first]
                evaluations[p[good]] += 1
                no_cascade[p[good & (cas == 4)]] = True
                early_out[p[good & early]] = True
                shadow[sh] = s_
            directional = kind == L.LIGHT_TYPE_DIRECTIONAL
            term = np.where(directional[:, None], term * shadow[:, None], term).astype(F)
            keep = ~stale[at]
            total[at[keep]] = total[at[keep]] + term[keep]
        finite = np.isfinite(total)
        if render_mode == 8:
            rgba = base.heat(n_p)
            factor[:], cascade[:], evaluations[:], no_cascade[:], early_out[:] = 1, NONE, 0, False, False
        else:
            degenerate = ~finite.all(axis=1)
            rgba = np.concatenate([np.where(finite, total, F(0)), np.ones((count, 1), F)], axis=1).astype(F)
    ok = ~stale
    init = 0 if clear else fill
    color = np.full((h * w, 4), init, np.uint32).view(F)
    walked = np.full(h * w, init, np.uint32)
    factor_plane = np.full(h * w, 0x3F800000 if clear else fill, np.uint32).view(F)
    cascade_plane = np.full(h * w, NONE if clear else fill, np.uint32)
    color[pix[ok]], walked[pix[ok]], factor_plane[pix[ok]], cascade_plane[pix[ok]] = rgba[ok], n_p[ok], factor[ok], cascade[ok]
    lit_plane = np.full(h * w, -1, np.int64)
    lit_plane[pix[ok]] = lit_first[ok]
    blockers_plane = np.full(h * w, -1, np.int64)
    blockers_plane[pix[ok]] = blockers_first[ok]
    stats = np.zeros(1, L.SHADE_STATS)[0]
    outside = c["outside"][pix]
    counts = (c["covered"].sum(), ok.sum(), c["unshaded"].sum(), c["stale"].sum() + stale.sum(), (outside & ok).sum(), (degenerate & ok).sum(),
              (textured & ok).sum(), (unserved & ok).sum())
    for name, v in zip(base.STATS, counts):
        stats[name] = v
    shadow_stats = np.zeros(1, L.SHADOW_STATS)[0]
    for name, v in zip(SHADOW_STATS, ((ok & (evaluations > 0)).sum(), (ok & no_cascade).sum(), (ok & early_out).sum(), evaluations[ok].sum())):
        shadow_stats[name] = v
    any_stale = bool(c["stale"].any() or stale.any())
    stale_plane = c["stale"].copy()
    stale_plane[pix[stale]] = True
    return dict(color=color.reshape(h, w, 4), lights_walked=walked.reshape(h, w), stats=stats, status=_lib.E_RANGE if any_stale else 0,
                shadow_factor=factor_plane.reshape(h, w), cascade=cascade_plane.reshape(h, w), shadow_stats=shadow_stats,
                lit=lit_plane.reshape(h, w), blockers=blockers_plane.reshape(h, w), stale=stale_plane.reshape(h, w))


def shadow64(rows, wp4, N, direction, inner_radius, xs, ys, maps, res, blocker_search_radius, normal_bias_scale, oriented_bias, cascade):
    """forward.frag:81-184, :423-445 in float64 with the true sin and cos for entries whose cascade (0..3) is given ->
    (lit taps of the filter or -1 where it returns early, knife: a tap coordinate within 2^-18 of a texel boundary or a z
    within one float32 ulp of a compared texel)"""
    D = np.float64
    n = len(rows)
    M = rows["light_projection_matrices"][np.arange(n), cascade].astype(D).reshape(n, 4, 4).transpose(0, 2, 1)  # row-major
    wp, Nn, d = wp4[:, :3].astype(D), N.astype(D), direction.astype(D)
    tx = 1.0 / res
    ndl = (Nn * d).sum(1)
    sp = wp + (tx * D(F(normal_bias_scale)) * np.clip(1.0 - ndl, 0.0, 1.0))[:, None] * Nn
    sp = sp + np.where(ndl > 0, -D(F(oriented_bias)), D(F(oriented_bias)))[:, None] * d
    c = np.einsum("nij,nj->ni", M, np.concatenate([sp, np.ones((n, 1))], axis=1))
    z = c[:, 2] / c[:, 3]
    u, v = (c[:, 0] / c[:, 3] + 1.0) * 0.5, (-c[:, 1] / c[:, 3] + 1.0) * 0.5
    inv_ws = 1.0 / rows["shadow_map_world_sizes"][np.arange(n), cascade].astype(D)
    light_uv = inner_radius.astype(D) * inv_ws
    sx, sy = xs + 0.5, ys + 0.5
    frac = lambda a: a - np.floor(a)  # noqa: E731
    theta = frac(D(F(52.9829189)) * frac(sx * D(F(0.06711056)) + sy * D(F(0.00583715)))) * 2.0 * D(PI)
    s, cs = np.sin(theta), np.cos(theta)
    origin = rows["shadow_map_indices"][np.arange(n), cascade].astype(np.int64) * res * res
    off = POISSON.astype(D)
    knife = np.zeros(n, bool)

    def near_edge(a):
        return np.abs(a - np.round(a)) < 2.0 ** -18

    def ulp_close(t):
        return np.abs(z - t.astype(D)) <= np.spacing(np.abs(t)).astype(D)

    rad = D(F(blocker_search_radius)) * inv_ws
    avg, count = np.zeros(n), np.zeros(n, np.int64)
    for ox, oy in off[:12]:
        su, sv = u + (cs * ox - s * oy) * rad * inv_ws, v + (s * ox + cs * oy) * rad * inv_ws
        knife |= near_edge(su * res) | near_edge(sv * res)
        t = maps[origin + np.clip(np.floor(sv * res), 0, res - 1).astype(np.int64) * res + np.clip(np.floor(su * res), 0, res - 1).astype(np.int64)]
        knife |= ulp_close(t)
        blocked = t.astype(D) > z
        avg += np.where(blocked, 1.0 - t.astype(D), 0.0)
        count += blocked
    early = (count == 0) | (count == 12)
    with np.errstate(all="ignore"):
        avg = avg / count
        fr = np.maximum(((1.0 - z) - avg) / avg * light_uv * inv_ws, tx)
    fr = np.where(early, tx, fr)
    lit = np.zeros(n, np.int64)
    for ox, oy in off:
        fx, fy = (u + (cs * ox - s * oy) * fr) * res - 0.5, (v + (s * ox + cs * oy) * fr) * res - 0.5
        knife |= near_edge(fx) | near_edge(fy)
        x0, y0 = np.floor(fx), np.floor(fy)
        for yy in (y0, y0 + 1):
            for xx in (x0, x0 + 1):
                t = maps[origin + np.clip(yy, 0, res - 1).astype(np.int64) * res + np.clip(xx, 0, res - 1).astype(np.int64)]
                knife |= ulp_close(t)
                lit += z >= t.astype(D)
    return np.where(early, -1, lit), knife
