"""orbit_fragments_shade restated in numpy float32 from the rules L1-L9 of include/orbit_abi_ext.h — an independent
restatement that shares nothing with orbit_amd/csrc/shade_common.h: the slice comes from the oracle's log2f and an exact
fused multiply-add built from float64, the walk runs position by position over all pixels at once, every float32
operation is numpy's (each rounded on its own).  `shade64` is the GLSL itself in float64, with a true pow(x, 5) and a
double log2: what the accuracy figures are measured against."""
import numpy as np

from orbit_amd import _lib
from orbit_amd import layouts as L

F = np.float32
NONE = 0xFFFFFFFF
EPS, PI = F(0.0001), F(3.14159265359)
STATS = ("covered_pixels", "written_pixels", "unshaded_pixels", "stale_pixels", "outside_pixels", "degenerate_pixels", "textured_pixels",
         "unserved_pixels")


def fma32(a, b, c):
    """float32 fma(a, b, c) of arrays, exactly: the product is exact in float64, the sum is rounded to odd there (the
    neighbour on the error's side when the float64 sum is inexact and even), and odd rounding survives the second one."""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0)
        even = (s.view(np.int64) & 1) == 0
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(inexact & even, np.nextafter(s, toward), s)
        return s.astype(F)


def f2u_sat(t):
    """uint(float): saturating, NaN -> 0"""
    t = np.asarray(t, F)
    with np.errstate(all="ignore"):
        out = np.where(t >= F(4294967296.0), np.uint64(NONE), np.where(t > 0, t, F(0)).astype(np.uint64))
    return np.where(t > 0, out, 0).astype(np.uint64)


def slices(oracle, vis, z_near, z_scale, z_bias):
    """L2's slice of every pixel of the (h, w) u64 buffer -> (h, w) uint64 (meaningless where the word is 0)"""
    d = (np.asarray(vis, np.uint64) >> np.uint64(32)).astype(np.uint32).view(F)
    with np.errstate(all="ignore"):
        z = F(z_near) / d
    uniq, inverse = np.unique(z.view(np.uint32), return_inverse=True)
    logs = np.array([oracle.log2f(float(v)) for v in uniq.view(F)], np.float64).astype(F)
    return f2u_sat(fma32(logs, F(z_scale), F(z_bias)))[inverse.reshape(z.shape)]


def gmax(x, y):
    return np.where(x < y, y, x).astype(F)


def gclamp(x, lo, hi):
    m = gmax(x, lo)
    return np.where(hi < m, hi, m).astype(F)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize(v):
    return v / np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])[..., None]


def heat(n):
    x = gclamp(n.astype(F) / F(32.0), F(0), F(1))
    r = np.where(x < F(0.7), F(4) * x - F(1.5), F(-4) * x + F(4.5))
    g = np.where(x < F(0.5), F(4) * x - F(0.5), F(-4) * x + F(3.5))
    b = np.where(x < F(0.3), F(4) * x + F(0.5), F(-4) * x + F(2.5))
    return np.stack([gclamp(c.astype(F), F(0), F(1)) for c in (r, g, b)] + [np.ones_like(x)], axis=-1)


def classify(oracle, vis, material, materials, lights, image, index_buffer, cluster_count, tile_size_px, z_scale, z_bias, z_near,
             material_count=None, light_count=None, index_capacity=None, slice_of=None):
    """L1 and L2 of every pixel -> dict of flat arrays: covered, unshaded, stale, live (to be written), outside, offset, n,
    and `indices` (the u32 list)"""
    vis = np.asarray(vis, np.uint64)
    h, w = vis.shape
    mats = np.ascontiguousarray(materials).view(np.uint8).reshape(-1)
    material_count = mats.nbytes // 80 if material_count is None else material_count
    light_count = np.ascontiguousarray(lights).view(np.uint8).size // 64 if light_count is None else light_count
    raw = np.ascontiguousarray(index_buffer).view(np.uint8).reshape(-1)
    indices = raw[4:4 + (len(raw) - 4) // 4 * 4].view(np.uint32)
    index_capacity = len(indices) if index_capacity is None else index_capacity
    img = np.ascontiguousarray(image).view(np.uint32).reshape(-1, 2)
    cx, cy, cz = (int(c) for c in cluster_count)
    covered = (vis != 0).reshape(-1)
    mat = np.asarray(material, np.uint32).reshape(-1)
    unshaded = covered & (mat == NONE)
    stale = covered & ~unshaded & (mat >= material_count)
    ys, xs = np.divmod(np.arange(h * w), w)
    tx, ty = xs // tile_size_px, ys // tile_size_px
    sl = (slices(oracle, vis, z_near, z_scale, z_bias) if slice_of is None else slice_of).reshape(-1)
    outside = (tx >= cx) | (ty >= cy) | (sl >= cz)
    cluster = np.where(outside, 0, tx + ty * cx + np.minimum(sl, cz - 1).astype(np.int64) * cx * cy)
    offset = np.where(outside, 0, img[cluster, 0]).astype(np.int64)
    n = np.where(outside, 0, np.minimum(img[cluster, 1], 256)).astype(np.int64)
    cand = covered & ~unshaded & ~stale
    over = cand & (offset + n > index_capacity)
    stale |= over
    cand &= ~over
    for i in range(int(n[cand].max()) if cand.any() else 0):
        walking = cand & (n > i)
        bad = np.zeros_like(walking)
        bad[walking] = indices[offset[walking] + i] >= light_count
        stale |= bad
        cand &= ~bad
    return dict(covered=covered, unshaded=unshaded, stale=stale, live=cand, outside=outside & cand, offset=offset, n=n, indices=indices,
                slice=sl)


def shade(oracle, vis, world_pos, normal, material, materials, lights, image, index_buffer, cluster_count, tile_size_px, z_scale, z_bias,
          luminance_cutoff, z_near, view_pos, render_mode=0, clear=True, fill=0, material_count=None, light_count=None,
          index_capacity=None):
    """-> dict(color (h, w, 4) float32, lights_walked (h, w) uint32, stats np[layouts.SHADE_STATS] row, status), as
    orbit_amd.raster.host_fragments_shade"""
    vis = np.asarray(vis, np.uint64)
    h, w = vis.shape
    c = classify(oracle, vis, material, materials, lights, image, index_buffer, cluster_count, tile_size_px, z_scale, z_bias, z_near,
                 material_count, light_count, index_capacity)
    live, n, offset, indices = c["live"], c["n"], c["offset"], c["indices"]
    mats = np.ascontiguousarray(materials).view(np.uint8).reshape(-1)
    mats = mats[:len(mats) // 80 * 80].view(L.MATERIAL)
    lts = np.ascontiguousarray(lights).view(np.uint8).reshape(-1)
    lts = lts[:len(lts) // 64 * 64].view(L.LIGHT)
    pix = np.flatnonzero(live)
    m = mats[np.asarray(material, np.uint32).reshape(-1)[pix]]
    textured = (m["texture_indices"] != NONE).any(axis=1)
    unserved = np.zeros(len(pix), bool)
    degenerate = np.zeros(len(pix), bool)
    n_p, off_p = n[pix], offset[pix]
    with np.errstate(all="ignore"):
        if render_mode == 8:
            rgba = heat(n_p)
        else:
            wp = np.asarray(world_pos, F).reshape(-1, 4)[pix, :3]
            N = np.asarray(normal, F).reshape(-1, 3)[pix]
            albedo, metallic, r = m["base_color"][:, :3].astype(F), m["metallic_factor"].astype(F), m["roughness_factor"].astype(F)
            V = normalize(np.asarray(view_pos, F)[None, :] - wp)
            total = m["emissive_factor"].astype(F).copy()
            cutoff = F(luminance_cutoff)
            for i in range(int(n_p.max()) if len(pix) else 0):
                at = np.flatnonzero(n_p > i)
                l = lts[indices[off_p[at] + i]]
                kind = l["light_type"]
                unserved[at] |= (kind == L.LIGHT_TYPE_SKY) | ((kind == L.LIGHT_TYPE_DIRECTIONAL) & (l["shadow_data_index"] != NONE))
                lit = (kind == L.LIGHT_TYPE_POINT) | (kind == L.LIGHT_TYPE_DIRECTIONAL)
                at, l, kind = at[lit], l[lit], kind[lit]
                if not len(at):
                    continue
                point = kind == L.LIGHT_TYPE_POINT
                lc = l["color"] * l["intensity"][:, None]
                Ld = l["position"] - wp[at]
                dist = np.sqrt(dot(Ld, Ld))
                Ld = Ld / dist[:, None]
                dist = gmax(dist, l["inner_radius"])
                d2 = dist * dist
                att = gmax(l["intensity"] / d2 - (cutoff * d2) / (l["outer_radius"] * l["outer_radius"]), F(0))
                Ld = np.where(point[:, None], Ld, l["direction"]).astype(F)
                att = np.where(point, att, F(1)).astype(F)
                Vv, Nn, al, me, ro = V[at], N[at], albedo[at], metallic[at], r[at]
                H = normalize(Vv + Ld)
                ndv, ndl = gmax(dot(Nn, Vv), EPS), gmax(dot(Nn, Ld), EPS)
                ndh, hv = gmax(dot(Nn, H), F(0)), gmax(dot(H, Vv), F(0))
                a = ro * ro
                a2 = a * a
                den = (ndh * ndh) * (a2 - F(1)) + F(1)
                den = (PI * den) * den
                D = a2 / gmax(den, EPS)
                rr = ro + F(1)
                k = (rr * rr) / F(8)
                G = (ndv / (ndv * (F(1) - k) + k)) * (ndl / (ndl * (F(1) - k) + k))
                f0 = F(0.04) * (F(1) - me)[:, None] + al * me[:, None]
                x = F(1) - hv
                p5 = ((x * x) * (x * x)) * x
                Fr = f0 + (F(1) - f0) * p5[:, None]
                spec = ((D * G)[:, None] * Fr) / ((F(4) * ndv) * ndl)[:, None]
                kD = (F(1) - Fr) * (F(1) - me)[:, None]
                total[at] = total[at] + ((((kD * al) / PI) + spec) * (lc * att[:, None])) * ndl[:, None]
            finite = np.isfinite(total)
            degenerate = ~finite.all(axis=1)
            rgba = np.concatenate([np.where(finite, total, F(0)), np.ones((len(pix), 1), F)], axis=1).astype(F)
    color = np.full((h * w, 4), 0 if clear else fill, np.uint32).view(F)
    walked = np.full(h * w, 0 if clear else fill, np.uint32)
    color[pix] = rgba
    walked[pix] = n_p
    stats = np.zeros(1, L.SHADE_STATS)[0]
    counts = (c["covered"].sum(), len(pix), c["unshaded"].sum(), c["stale"].sum(), c["outside"].sum(), degenerate.sum(), textured.sum(),
              unserved.sum())
    for name, v in zip(STATS, counts):
        stats[name] = v
    return dict(color=color.reshape(h, w, 4), lights_walked=walked.reshape(h, w), stats=stats, status=_lib.E_RANGE if c["stale"].any() else 0,
                live=live.reshape(h, w), classified=c)


def shade64(vis, world_pos, normal, material, materials, lights, image, index_buffer, cluster_count, tile_size_px, z_scale, z_bias,
            luminance_cutoff, z_near, view_pos, pixels):
    """forward.frag's render_mode 0 in float64 for the flat pixel indices `pixels` (all in range: no stale walk): true pow(x,
    5.0), double log2 -> (rgb (len, 3) float64, slice (len,) int64)"""
    vis = np.asarray(vis, np.uint64)
    h, w = vis.shape
    D_ = np.float64
    d = (vis.reshape(-1)[pixels] >> np.uint64(32)).astype(np.uint32).view(F).astype(D_)
    cx, cy, cz = (int(c) for c in cluster_count)
    with np.errstate(all="ignore"):
        t = np.log2(D_(F(z_near)) / d) * D_(F(z_scale)) + D_(F(z_bias))
        sl = np.where(t > 0, np.minimum(np.nan_to_num(t, nan=0.0, posinf=2.0 ** 32), 2.0 ** 32 - 1), 0).astype(np.int64)
    ys, xs = np.divmod(pixels, w)
    tx, ty = xs // tile_size_px, ys // tile_size_px
    outside = (tx >= cx) | (ty >= cy) | (sl >= cz)
    img = np.ascontiguousarray(image).view(np.uint32).reshape(-1, 2)
    cluster = np.where(outside, 0, tx + ty * cx + np.minimum(sl, cz - 1) * cx * cy)
    offset = np.where(outside, 0, img[cluster, 0]).astype(np.int64)
    n = np.where(outside, 0, np.minimum(img[cluster, 1], 256)).astype(np.int64)
    raw = np.ascontiguousarray(index_buffer).view(np.uint8).reshape(-1)
    indices = raw[4:4 + (len(raw) - 4) // 4 * 4].view(np.uint32)
    mats = np.ascontiguousarray(materials).view(np.uint8).reshape(-1)
    m = mats[:len(mats) // 80 * 80].view(L.MATERIAL)[np.asarray(material, np.uint32).reshape(-1)[pixels]]
    lts = np.ascontiguousarray(lights).view(np.uint8).reshape(-1)
    lts = lts[:len(lts) // 64 * 64].view(L.LIGHT)
    wp = np.asarray(world_pos, F).reshape(-1, 4)[pixels, :3].astype(D_)
    N = np.asarray(normal, F).reshape(-1, 3)[pixels].astype(D_)
    albedo, metallic, r = m["base_color"][:, :3].astype(D_), m["metallic_factor"].astype(D_), m["roughness_factor"].astype(D_)
    norm = lambda v: v / np.linalg.norm(v, axis=1)[:, None]  # noqa: E731
    eps, pi = D_(F(0.0001)), D_(F(3.14159265359))
    with np.errstate(all="ignore"):
        V = norm(np.asarray(view_pos, F).astype(D_)[None, :] - wp)
        total = m["emissive_factor"].astype(D_).copy()
        for i in range(int(n.max()) if len(pixels) else 0):
            at = np.flatnonzero(n > i)
            l = lts[indices[offset[at] + i]]
            kind = l["light_type"]
            lit = (kind == L.LIGHT_TYPE_POINT) | (kind == L.LIGHT_TYPE_DIRECTIONAL)
            at, l, kind = at[lit], l[lit], kind[lit]
            if not len(at):
                continue
            point = kind == L.LIGHT_TYPE_POINT
            inten = l["intensity"].astype(D_)
            lc = l["color"].astype(D_) * inten[:, None]
            Ld = l["position"].astype(D_) - wp[at]
            dist = np.linalg.norm(Ld, axis=1)
            Ld = Ld / dist[:, None]
            dist = np.maximum(dist, l["inner_radius"].astype(D_))
            att = np.maximum(inten / dist ** 2 - D_(F(luminance_cutoff)) * dist ** 2 / l["outer_radius"].astype(D_) ** 2, 0.0)
            Ld = np.where(point[:, None], Ld, l["direction"].astype(D_))
            att = np.where(point, att, 1.0)
            Vv, Nn, al, me, ro = V[at], N[at], albedo[at], metallic[at], r[at]
            H = norm(Vv + Ld)
            ndv, ndl = np.maximum((Nn * Vv).sum(1), eps), np.maximum((Nn * Ld).sum(1), eps)
            ndh, hv = np.maximum((Nn * H).sum(1), 0.0), np.maximum((H * Vv).sum(1), 0.0)
            a2 = (ro * ro) ** 2
            den = ndh * ndh * (a2 - 1.0) + 1.0
            Dg = a2 / np.maximum(pi * den * den, eps)
            k = (ro + 1.0) ** 2 / 8.0
            G = (ndv / (ndv * (1.0 - k) + k)) * (ndl / (ndl * (1.0 - k) + k))
            f0 = 0.04 * (1.0 - me)[:, None] + al * me[:, None]
            Fr = f0 + (1.0 - f0) * np.power(1.0 - hv, 5.0)[:, None]
            spec = (Dg * G)[:, None] * Fr / (4.0 * ndv * ndl)[:, None]
            kD = (1.0 - Fr) * (1.0 - me)[:, None]
            total[at] += (kD * al / pi + spec) * (lc * att[:, None]) * ndl[:, None]
    return total, sl
