"""orbit_fragments_shade_sky restated in numpy from forward.frag:378-405, skybox.vert / skybox.frag and the rules K1-K10 of
include/orbit_abi_ext.h — an independent restatement that shares nothing with orbit_amd/csrc/sky_common.h: the walk
position by position over all pixels at once, the cubes through env_map_ref.Cube (bordered faces found geometrically, not
the mirror's integer fold), the table by its own bilinear tap, the ray from the pixel centre.  The float type T is a
parameter.  With T = float32 every operation is numpy's, rounded on its own: what the mirror must give byte for byte.  With
T = float64 the sky term, the skybox and the light sum are the GLSL in double precision on the stored fp16 texels: the
yardstick of tools/count_fragments_shade_sky.py.  (The point and directional terms and the shadow factor come from
fragments_shade_shadowed_ref in float32 either way: their own distance is §4.25's and §4.26's figure.)"""
import numpy as np

import env_map_ref as er
import fragments_shade_ref as base
import fragments_shade_shadowed_ref as sref
from orbit_amd import _lib
from orbit_amd import layouts as L

F, D = np.float32, np.float64
NONE = 0xFFFFFFFF
SKY_STATS = ("sky_evaluations", "sky_lit_pixels", "skybox_pixels", "bad_directions")


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def gmax(x, y):
    return np.where(x < y, y, x)


def gmin(x, y):
    return np.where(y < x, y, x)


def texel(f, n):
    """clamp(int(f), 0, n - 1) of floored floats, the conversion saturating, NaN -> 0"""
    with np.errstate(all="ignore"):
        return np.where(f > 0, np.where(f >= n, n - 1, np.where(np.isfinite(f), f, 0)), 0).astype(np.int64)


class Environment:
    """the three images of a call as K4-K6 read them"""

    def __init__(self, env, T):
        self.T = T
        self.irradiance = er.Cube(np.asarray(env["irradiance"], np.uint16).reshape(-1)[:24 * env["irradiance_size"] ** 2], env["irradiance_size"], 1, T)
        levels, size = env["prefiltered_levels"], env["prefiltered_size"]
        texels = sum(6 * max(1, size >> m) ** 2 for m in range(levels))
        self.prefiltered = er.Cube(np.asarray(env["prefiltered"], np.uint16).reshape(-1)[:4 * texels], size, levels, T)
        self.levels = levels
        n = env["brdf_size"]
        self.n = n
        with np.errstate(all="ignore"):
            self.brdf = np.asarray(env["brdf"], np.uint16).reshape(-1)[:2 * n * n].view(np.float16).astype(T).reshape(n, n, 2)

    def table(self, u, v):
        """K6: LinearClamp at (u, v) -> (n, 2)"""
        T, n, t = self.T, self.n, self.brdf
        with np.errstate(all="ignore"):
            sx, sy = u * T(n) - T(0.5), v * T(n) - T(0.5)
            flx, fly = np.floor(sx), np.floor(sy)
            fx, fy = (sx - flx)[:, None], (sy - fly)[:, None]
            gx, gy = T(1) - fx, T(1) - fy
            x0, x1, y0, y1 = texel(flx, n), texel(flx + T(1), n), texel(fly, n), texel(fly + T(1), n)
            return (t[y0, x0] * gx + t[y0, x1] * fx) * gy + (t[y1, x0] * gx + t[y1, x1] * fx) * fy


def sky_terms(env, N, V, albedo, metallic, r, lc, ao):
    """forward.frag:378-405 per entry (all arrays of T) -> the term (n, 3), E4's bad directions per entry (n,)"""
    T = env.T
    with np.errstate(all="ignore"):
        nv = dot3(N, V)
        R = V - (T(2) * nv)[:, None] * N  # reflect(view_direction, normal)
        R[:, 1] = R[:, 1] * T(-1)
        ndv0 = gmax(nv, T(0))
        f0 = T(0.04) * (T(1) - metallic)[:, None] + albedo * metallic[:, None]
        x = gmin(gmax(T(1) - ndv0, T(0)), T(1))
        p5 = ((x * x) * (x * x)) * x
        kS = f0 + (gmax((T(1) - r)[:, None], f0) - f0) * p5[:, None]
        kD = (T(1) - kS) * (T(1) - metallic)[:, None]
        irr, bad_n = env.irradiance.sample([N[:, 0], N[:, 1], N[:, 2]], np.zeros(len(N), T))
        diffuse = irr * albedo
        lod = r * T(env.levels - 1)
        refl, bad_r = env.prefiltered.sample([R[:, 0], R[:, 1], R[:, 2]], lod)
        ab = env.table(ndv0, r)
        spec = refl * (kS * ab[:, 0:1] + ab[:, 1:2])
        term = ((kD * diffuse + spec) * lc) * ao[:, None]
    return term.astype(T), bad_n.astype(np.int64) + bad_r.astype(np.int64)


def skybox(sky, skybox_lod, basis, width, height, xs, ys, T):
    """skybox.vert / skybox.frag of the pixels (xs, ys): the ray through the pixel centre -> rgba (n, 4), bad (n,)"""
    cube = er.Cube(np.asarray(sky["cube"], np.uint16).reshape(-1)[:24 * sum(max(1, sky["size"] >> m) ** 2 for m in range(sky["levels"]))],
                   sky["size"], sky["levels"], T)
    bx, by, bz = (np.asarray(b, F).astype(T) for b in basis)
    with np.errstate(all="ignore"):
        cx = (T(2) * (xs.astype(T) + T(0.5))) / T(width) - T(1)
        cy = T(1) - (T(2) * (ys.astype(T) + T(0.5))) / T(height)
        d = [(cx * bx[k] + cy * by[k]) + bz[k] for k in range(3)]
        length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        d = [c / length for c in d]
        rgb, bad = cube.sample(d, np.full(len(xs), F(skybox_lod)).astype(T))
    rgb = np.where(np.isfinite(rgb), rgb, T(0))
    return np.concatenate([rgb, np.ones((len(xs), 1), T)], axis=1).astype(T), bad


def shade(oracle, vis, world_pos, normal, material, materials, lights, image, index_buffer, cluster_count, tile_size_px, z_scale, z_bias,
          luminance_cutoff, z_near, view_pos, shadows, shadow_maps, shadow_resolution, blocker_search_radius, normal_bias_scale,
          oriented_bias, env=None, sky=None, skybox_lod=0.0, basis=None, ao=None, shadow_index_base=0, shadow_count=None,
          shadow_map_count=None, render_mode=0, clear=True, fill=0, material_count=None, light_count=None, index_capacity=None, T=F):
    """-> the dict of orbit_amd.raster.host_fragments_shade_sky (every optional output present; color of type T)"""
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
    environment = Environment(env, T) if env is not None and render_mode == 0 else None
    pix = np.flatnonzero(c["live"])
    ys, xs = np.divmod(pix, w)
    m = mats[np.asarray(material, np.uint32).reshape(-1)[pix]]
    textured = (m["texture_indices"] != NONE).any(axis=1)
    count = len(pix)
    unserved, degenerate, stale = np.zeros(count, bool), np.zeros(count, bool), np.zeros(count, bool)
    factor, cascade = np.ones(count, F), np.full(count, NONE, np.uint32)
    evaluations, sky_evaluations, sky_bad = np.zeros(count, np.int64), np.zeros(count, np.int64), np.zeros(count, np.int64)
    no_cascade, early_out = np.zeros(count, bool), np.zeros(count, bool)
    n_p, off_p = n[pix], offset[pix]
    wp4 = np.asarray(world_pos, F).reshape(-1, 4)[pix]
    N = np.asarray(normal, F).reshape(-1, 3)[pix]
    with np.errstate(all="ignore"):
        albedo, metallic, r = m["base_color"][:, :3].astype(F), m["metallic_factor"].astype(F), m["roughness_factor"].astype(F)
        eye = np.asarray(view_pos, F)[None, :]
        V = base.normalize(eye - wp4[:, :3])
        VT = V if T is F else (lambda v: v / np.sqrt(dot3(v, v))[:, None])(eye.astype(T) - wp4[:, :3].astype(T))
        occlusion = np.ones(count, T) if ao is None else gmin(T(1), np.asarray(ao, F).reshape(-1)[pix].astype(T)).astype(T)
        total = m["emissive_factor"].astype(T).copy()
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
            is_sky = kind == L.LIGHT_TYPE_SKY
            if environment is None:
                unserved[at] |= is_sky  # K1: skipped and counted as before
            elif is_sky.any():
                p = at[is_sky]
                lc = (l["color"][is_sky] * l["intensity"][is_sky][:, None]).astype(T)
                term, bad_dirs = sky_terms(environment, N[p].astype(T), VT[p], albedo[p].astype(T), metallic[p].astype(T), r[p].astype(T), lc,
                                           occlusion[p])
                total[p] = total[p] + term
                sky_evaluations[p] += 1
                sky_bad[p] += bad_dirs
            lit = (kind == L.LIGHT_TYPE_POINT) | (kind == L.LIGHT_TYPE_DIRECTIONAL)
            at, l, kind, shadowed, row = at[lit], l[lit], kind[lit], shadowed[lit], row[lit]
            if not len(at):
                continue
            term = sref.light_terms(l, wp4[at, :3], N[at], V[at], albedo[at], metallic[at], r[at], cutoff)
            shadow = np.ones(len(at), F)
            sh = np.flatnonzero(shadowed)
            if len(sh):
                p = at[sh]
                s_, cas, bad, early, _, _ = sref.evaluate(rows[row[sh]], wp4[p], N[p], l["direction"][sh], l["inner_radius"][sh], xs[p], ys[p], maps,
                                                          shadow_map_count, res, blocker_search_radius, normal_bias_scale, oriented_bias)
                stale[p[bad]] = True
                good = ~bad
                first = good & (evaluations[p] == 0)
                factor[p[first]], cascade[p[first]] = s_[first], cas[first]
                evaluations[p[good]] += 1
                no_cascade[p[good & (cas == 4)]] = True
                early_out[p[good & early]] = True
                shadow[sh] = s_
            directional = kind == L.LIGHT_TYPE_DIRECTIONAL
            term = np.where(directional[:, None], term * shadow[:, None], term).astype(F)
            keep = ~stale[at]
            total[at[keep]] = total[at[keep]] + term[keep].astype(T)
        finite = np.isfinite(total)
        if render_mode == 8:
            rgba = base.heat(n_p).astype(T)
            factor[:], cascade[:], evaluations[:], no_cascade[:], early_out[:] = 1, NONE, 0, False, False
        else:
            degenerate = ~finite.all(axis=1)
            rgba = np.concatenate([np.where(finite, total, T(0)), np.ones((count, 1), T)], axis=1).astype(T)
    ok = ~stale
    init = 0 if clear else fill
    color = np.full((h * w, 4), init, np.uint32).view(F).astype(T) if T is not F else np.full((h * w, 4), init, np.uint32).view(F)
    walked = np.full(h * w, init, np.uint32)
    factor_plane = np.full(h * w, 0x3F800000 if clear else fill, np.uint32).view(F)
    cascade_plane = np.full(h * w, NONE if clear else fill, np.uint32)
    color[pix[ok]], walked[pix[ok]], factor_plane[pix[ok]], cascade_plane[pix[ok]] = rgba[ok], n_p[ok], factor[ok], cascade[ok]
    sky_stats = np.zeros(1, L.SKY_STATS)[0]
    box_mask = np.zeros(h * w, bool)
    box_bad = 0
    if sky is not None and render_mode == 0:  # K9
        open_ = np.flatnonzero(vis.reshape(-1) == 0)
        by, bx = np.divmod(open_, w)
        rgba_box, bad_box = skybox(sky, skybox_lod, basis, w, h, bx, by, T)
        color[open_] = rgba_box
        box_mask[open_] = True
        box_bad = int(bad_box.sum())
        sky_stats["skybox_pixels"] = len(open_)
    sky_stats["sky_evaluations"], sky_stats["sky_lit_pixels"] = sky_evaluations[ok].sum(), (ok & (sky_evaluations > 0)).sum()
    sky_stats["bad_directions"] = int(sky_bad[ok].sum()) + box_bad
    stats = np.zeros(1, L.SHADE_STATS)[0]
    outside = c["outside"][pix]
    counts = (c["covered"].sum(), ok.sum(), c["unshaded"].sum(), c["stale"].sum() + stale.sum(), (outside & ok).sum(), (degenerate & ok).sum(),
              (textured & ok).sum(), (unserved & ok).sum())
    for name, v in zip(base.STATS, counts):
        stats[name] = v
    shadow_stats = np.zeros(1, L.SHADOW_STATS)[0]
    for name, v in zip(sref.SHADOW_STATS, ((ok & (evaluations > 0)).sum(), (ok & no_cascade).sum(), (ok & early_out).sum(), evaluations[ok].sum())):
        shadow_stats[name] = v
    any_stale = bool(c["stale"].any() or stale.any())
    lit_mask = np.zeros(h * w, bool)
    lit_mask[pix[ok & (sky_evaluations > 0)]] = True
    return dict(color=color.reshape(h, w, 4), lights_walked=walked.reshape(h, w), stats=stats, status=_lib.E_RANGE if any_stale else 0,
                shadow_factor=factor_plane.reshape(h, w), cascade=cascade_plane.reshape(h, w), shadow_stats=shadow_stats, sky_stats=sky_stats,
                sky_lit=lit_mask.reshape(h, w), skybox=box_mask.reshape(h, w))


def skybox_matrix_basis(orientation, fov_y, aspect):
    """K9's basis from the reference's own matrix product, skybox_view_projection_matrix = perspective_infinite_reverse_rh(
    fov_y, aspect, z_near) * inverse(Mat4::from_quat(orientation)) (forward.rs:471-472), in float64: the rays through clip
    points (1, 0), (0, 1) and (0, 0) are found by inverting the matrix's upper-left 3 x 3 rows for x, y and w."""
    x, y, z, w = (float(v) for v in orientation)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    f = 1.0 / np.tan(0.5 * fov_y)
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1], P[3, 2], P[2, 3] = f / aspect, f, -1.0, 0.01
    view = np.eye(4)
    view[:3, :3] = R
    M = P @ np.linalg.inv(view)
    A = M[[0, 1, 3], :3]  # clip x, y, w of a direction v (translation-free)
    inv = np.linalg.inv(A)
    centre = inv @ np.array([0.0, 0.0, 1.0])
    return inv @ np.array([1.0, 0.0, 1.0]) - centre, inv @ np.array([0.0, 1.0, 1.0]) - centre, centre
