"""Hostile inputs for the pass-2 HiZ test (occlusion_test -> project_sphere -> hiz_sample -> footprint_min) and a
census of what they exercise.

Shared by tests/test_hiz_edges_cpu.py (census floors, oracle == numpy restatement, oracle == the reference's binaries),
tests/test_hiz_edges_gpu.py (every kernel path against the oracle) and tests/golden/make_spirv_vectors.py `hiz_edges`.

`hostile_scene` mixes degenerate and non-finite geometry into a scenes.make_scene scene and adds two ladders of finite
spheres whose projected size sweeps every mip level; `hostile_depth` is a make_depth buffer with arbitrary bit patterns
and planted blocks of NaN / +inf / -inf / negative / denormal texels; `census` classifies, from the intermediates
tests/np_restatement.py exposes (the reference side only — nothing of the product is asked), the rows of a stage that
reach the occlusion test.  The floors the CPU tests hold every case to are a condition on these INPUTS.

Two classes are there because a one-line mutation of orbit_device.h went unnoticed without them: `cullable_tie_decides`
(`>=` against `>` in `cullable`: rungs whose near point is exactly on the near plane — which is also where the task
shader's binary, whose sums are not fused, parts from the cull shaders') and `collapsed_level_culls` (the
max(dim >> level, 1) of a level with a collapsed side: the *_floor cases, whose upper levels hold depths that cull).
"""
import numpy as np

import np_restatement as npr
import scenes as sc
from orbit_amd import layouts as L

F = np.float32
ORTHO = dict(p00=1.0 / 16, p11=1.0 / 16, z_near=0.7, z_far=61.3)
KINDS = ("nan", "pinf", "ninf", "negative", "denormal", "wall")
_BITS = dict(nan=0x7FC00001, pinf=0x7F800000, ninf=0xFF800000, negative=0xBE800000, denormal=0x00000123)
WALL = {False: 0.002, True: 0.85}  # by `ortho`: a depth in the middle of the range of `closest`, so that it decides both ways

# classes that cannot occur, or that a kind of case is not there for, with the reason (the floors skip them; census()
# still counts them)
IMPOSSIBLE = {
    "not_cullable@ortho": "the orthographic branch has no near-plane condition: cullable is constant true",
    "cullable_tie_decides@ortho": "the orthographic branch has no near-plane condition",
    "cullable_tie_decides@1x1": "a sphere whose near point is on the near plane has closest = 1 or so, above the one finite texel",
    "collapsed_level_culls@hostile": "under hostile texels a level with a collapsed side is the minimum of regions with a "
                                     "negative, -inf or NaN texel in them and culls by chance at most: the *_floor cases hold this class",
    "closest_inf@persp": "cullable bounds the divisor z - r below by z_near: closest <= 1",
    "closest_nan@persp": "needs z = +inf under an infinite radius, but an infinite centre or matrix entry meets a zero of the "
                         "view matrix or of the row (0 0 0 1) first: NaN, which is not cullable",
    "uv_outside@ortho": "the orthographic branch clamps its bounds to [-1, 1] before u, v are formed",
    "lod_above_top@ortho": "clamped bounds make width <= max(w0, h0) = 2^(mips - 1): lod <= mips - 1",
    "lod_pinf": "width = +inf needs an aabb quotient that overflows binary32; no finite sphere of these scenes has one, "
                "and a non-finite one gives NaN first (counted under lod_above_top should it ever occur)",
}


def screen_of(w0, h0):
    """A screen whose pyramid is w0 x h0 (level 0 is half the next power of two of each side)."""
    side = lambda d: 1 if d == 1 else d + d // 4 if d >= 8 else d + 1  # noqa: E731
    return side(w0), side(h0)


def planted_rects(w0, h0):
    """uv rectangles (u0, u1, v0, v1) of the planted blocks: six along the longer axis, each 10 % of it (at least six
    level-0 texels, that axis having 64 or more), half of the shorter axis (all of it below 16 texels) — so each
    survives the min-reduction onto several upper levels.  None on a pyramid too small to hold them."""
    if max(w0, h0) < 64:
        return {}
    across = (0.25, 0.75) if min(w0, h0) >= 16 else (0.0, 1.0)
    out = {}
    for k, kind in enumerate(KINDS):
        a, b = 0.06 + 0.15 * k, 0.16 + 0.15 * k
        out[kind] = (a, b) + across if w0 >= h0 else across + (a, b)
    return out


def hostile_depth(seed, W, H, cam, share=0.2, ortho=False, floor=False):
    """make_depth with `share` of the texels replaced by arbitrary bit patterns and the blocks of planted_rects (of
    this screen's pyramid) set to NaN, +inf, -inf, a negative and a denormal value and to WALL[ortho]; a screen of one
    texel is that wall.  The first two rows' and columns' corner stays as make_depth left it — a NaN there owns the top
    of the chain (gmin keeps its first operand) — in the orthographic cases, where the carriers of hostile_scene sample
    the top level; in the perspective cases the corner texel IS NaN and with it the first texel of every level.
    `floor`: the tame counterpart instead (below) — the hostile geometry of a *_floor case meets finite upper levels."""
    d = sc.make_depth(seed, W, H, cam)
    if W * H == 1:
        return np.full((1, 1), WALL[ortho], F)
    if floor:
        # the tame counterpart: nothing below the wall, only the +inf block planted — so that the upper levels, down
        # to those where one side has collapsed to 1, hold finite depths that still cull (under hostile texels every
        # upper level is the minimum of a region with a negative one in it, and a stray sample changes nothing)
        d = np.maximum(d, F(WALL[ortho]))
        u0, u1, v0, v1 = planted_rects(*npr_pyramid_size(W, H))["pinf"]
        d[int(np.floor(v0 * H)):int(np.ceil(v1 * H)), int(np.floor(u0 * W)):int(np.ceil(u1 * W))] = np.inf
        if not ortho:
            d[0, 0] = np.nan
        return np.ascontiguousarray(d)
    idx = np.arange(W * H)
    rnd = (sc.rnd_u64(seed, 66, idx) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(F).reshape(H, W)
    pick = (sc.rnd_f32(seed, 67, idx) < F(share)).reshape(H, W)
    pick[:2, :2] = False
    d = np.where(pick, rnd, d).astype(F)
    if not ortho:
        d[0, 0] = np.nan
    desc = npr_pyramid_size(W, H)
    for kind, (u0, u1, v0, v1) in planted_rects(*desc).items():
        x0, x1 = int(np.floor(u0 * W)), int(np.ceil(u1 * W))
        y0, y1 = int(np.floor(v0 * H)), int(np.ceil(v1 * H))
        d[y0:y1, x0:x1] = F(WALL[ortho]) if kind == "wall" else np.array([_BITS[kind]], np.uint32).view(F)[0]
    return np.ascontiguousarray(d)


def npr_pyramid_size(W, H):
    """Level 0 of the pyramid of a W x H screen (DepthPyramid::new: half the next power of two of each side)."""
    npot = lambda v: 1 << max(int(v) - 1, 0).bit_length()  # noqa: E731
    return max(npot(W) // 2, 1), max(npot(H) // 2, 1)


def _cycle(values, n):
    return [values[k % len(values)] for k in range(n)]


def _sphere_kinds():
    nan, inf = np.nan, np.inf
    # (component, value): 0-2 a centre component, 3 the radius
    return [(0, inf), (1, nan), (2, -inf), (3, inf), (3, nan), (3, 0.0), (3, -0.75), (3, 1e-30), (3, 1e30), (3, 1e6),
            (0, nan), (1, -inf), (2, inf), (3, -inf)]


def _merge(a, b):
    """Scene b appended to scene a (its meshes, meshlets, entities and visibility words after a's; a's materials)."""
    na, ma, wa = len(a.entities), len(a.meshlets), a.vis_words
    mi = b.mesh_infos.copy()
    mi["mesh_lods"][:, :, 0] += (mi["mesh_lods"][:, :, 1] > 0) * np.uint32(ma)
    draws = b.entity_draws.copy()
    draws["entity_index"] += na
    draws["mesh_index"] += len(a.mesh_infos)
    draws["visibility_offset"] += wa
    return sc.Scene(np.concatenate([a.entity_draws, draws]), np.concatenate([a.entities, b.entities]),
                    np.concatenate([a.mesh_infos, mi]), np.concatenate([a.meshlets, b.meshlets]), a.materials,
                    wa + b.vis_words, a.lod0_meshlets + b.lod0_meshlets, dict(a.meta))


def _tie(d, s, z_near):
    """(depth, model-space radius rho) next to (d, (d - z_near) / s) with fma(rho, s, z_near) == depth in binary32 and
    depth / s exact (a carrier's rung is stored divided by its scale)."""
    rho = F((d - float(F(z_near))) / s)
    for _ in range(64):
        depth = npr.fma32(rho, F(s), F(z_near))[()]
        if F(F(depth / F(s)) * F(s)) == depth:
            return float(depth), float(rho)
        rho = np.nextafter(rho, F(np.inf))
    raise AssertionError("no radius puts the near point on the near plane")


def _log_uniform(rng, lo, hi, count):
    """2^e (1 + m): log-uniform in steps, from exact operations only (the same on every host)."""
    e = rng.integers(int(np.floor(np.log2(lo))), int(np.ceil(np.log2(hi))), count)
    return np.clip(np.ldexp(1.0 + rng.random(count), e), lo, hi)


# what the rungs of a ladder are, twenty at a time: a `sweep` rung takes the next size of the ladder; a `probe` is aimed
# into a planted block of hostile_depth; an `edge` rung sits across a border of the screen; a `tangent` one is a hair
# from touching the eye (perspective: the projection grows without bound); a `poison` rung is still `cullable` but not
# finite downstream; a `tie` rung (perspective) has its near point EXACTLY on the near plane: z == fma(radius, scale,
# z_near), the equality `cullable` decides — so close that it samples the top level, whose texel is NaN there
_E_TABLE = ["sweep", "poison", "sweep", "probe", "sweep", "tangent", "sweep", "edge", "sweep", "poison",
            "sweep", "probe", "sweep", "poison", "sweep", "tie", "sweep", "probe", "sweep", "poison"]
_M_TABLE = ["sweep", "poison", "probe", "probe", "sweep", "tangent", "sweep", "edge", "probe", "probe",
            "sweep", "poison", "sweep", "edge", "sweep", "probe", "sweep", "tie", "sweep", "probe"]
# (component, value): a centre whose square overflows (perspective: NaN u, v), a negated radius (NaN lod; orthographic:
# the height decides the level), radius 0 (lod = -inf), radius inf (orthographic: closest = inf), an infinite centre
# (0 x inf in the matrix product: NaN everywhere)
_POISON = [(0, 1e30), (3, "negate"), (3, 0.0), (3, np.inf), (0, np.inf), (3, "negate"), (3, 0.0), (3, np.inf), (1, -1e25),
           (1, -np.inf), (0, -np.inf), (1, 1e25)]


def hostile_scene(seed, n, pyramid=(256, 128), ortho=False, cam=None, fractions=(0.5, 0.2, 0.15),
                  meshlets_per_mesh=((1, 40), (24, 70)), lods=3):
    """Two make_scene scenes with LOD chains, merged (one mesh per entity), of `n` entities, with, by share of the
    entities (`fractions`):
    - an ENTITY ladder: mesh spheres placed in view space whose projected size sweeps from under one texel to over the
      longer side of `pyramid` (_E_TABLE);
    - CARRIERS of a MESHLET ladder of the same kind (_M_TABLE): the entities of the second scene (meshes of
      meshlets_per_mesh[1] meshlets), whose own sphere is too large to be culled (the camera is inside it) and whose
      model matrix is the inverse view matrix times a scale — affine, so the evaluation's short cut is on —, every
      meshlet of theirs a rung;
    - hostile entities: projective model matrices, inf / NaN translations, zero, negative, 1e30 and 1e-30 scales, and
      scales that put the camera inside the entity's and its meshlets' spheres;
    and, over everything that is no rung: meshlet and mesh spheres with inf / NaN centre components and radius inf, NaN,
    0, negative, 1e-30 and huge.  The camera must not be rotated (the ladders are placed by translation)."""
    cam = camera() if cam is None else cam
    assert np.array_equal(np.asarray(cam.view)[:3, :3], np.eye(3, dtype=F))
    n_e, n_c, n_h = (int(n * f) for f in fractions)
    scene = _merge(sc.make_scene(seed, n - n_c, meshlets_per_mesh=meshlets_per_mesh[0], lods=lods),
                   sc.make_scene(seed + 7919, n_c, meshlets_per_mesh=meshlets_per_mesh[1], lods=lods))
    rng = np.random.default_rng(seed)
    w0, h0 = pyramid
    mips = npr.pyramid_levels(w0, h0)[0]
    proj = ORTHO if ortho else dict(p00=cam.p00, p11=cam.p11, z_near=cam.z_near)
    sr = proj["p00"]
    # level-0 texels per unit of r (of r / z in perspective).  Orthographic: the reference forms v0 from the lower and v1
    # from the upper bound, so `height` is negative and the width alone decides the level — unless the radius is negative
    texel = sr * w0 if ortho else max(proj["p00"] * w0, proj["p11"] * h0)
    tall_ortho = ortho and h0 > w0
    rects = planted_rects(w0, h0)
    rects = list(rects.values()) + ([rects["wall"]] * 2 if rects else [])
    eye = -np.asarray(cam.view, np.float64)[:3, 3]  # the camera's position

    seen = {}

    def rungs(count, table, scales):
        """view-space spheres (x, y, z, r) for rungs that will live under the scale(s) `scales`."""
        scales = np.broadcast_to(np.asarray(scales, np.float64), (count,))
        kind = np.array(_cycle(table, count))
        nth = np.zeros(count, np.int64)  # the how-manieth of its kind a rung is, over all calls
        for name in sorted(set(table)):
            got = int((kind == name).sum())
            nth[kind == name] = seen.get(name, 0) + np.arange(got)
            seen[name] = seen.get(name, 0) + got
        d = _log_uniform(rng, 3.0, 50.0, count)
        t = np.ldexp(1.0, -2) * 2.0 ** ((mips + 2.5) * ((nth * 0.6180339887498949) % 1.0))  # level-0 texels across
        u, v = -0.1 + 1.2 * rng.random(count), -0.1 + 1.2 * rng.random(count)
        small = np.ldexp(1.0 + rng.random(count), rng.integers(-2, 2, count))  # 0.25 .. 4 texels
        edge, side = kind == "edge", nth % 4
        u = np.where(edge & (side == 0), 0.0, np.where(edge & (side == 1), 1.0, u))
        v = np.where(edge & (side == 2), 0.0, np.where(edge & (side == 3), 1.0, v))
        t = np.where(edge, small, t)
        if rects:
            probe = kind == "probe"
            rc = np.array(rects)[nth % len(rects)]
            u = np.where(probe, rc[:, 0] + (rc[:, 1] - rc[:, 0]) * (0.2 + 0.6 * rng.random(count)), u)
            v = np.where(probe, rc[:, 2] + (rc[:, 3] - rc[:, 2]) * (0.2 + 0.6 * rng.random(count)), v)
            t = np.where(probe, small, t)
        if ortho:
            x, y, r = (2 * u - 1) / sr, (1 - 2 * v) / sr, t / texel
            if tall_ortho:  # three sweep rungs of four reach the levels above log2(w0) through the height
                r = np.where((kind == "sweep") & (nth % 4 != 0), -t / (sr * h0), r)
        else:
            x, y, r = (2 * u - 1) * d / proj["p00"], (1 - 2 * v) * d / proj["p11"], t * d / texel
            r = np.where(kind == "tangent", (d - proj["z_near"]) * (1.0 - np.ldexp(1.0, -(1 + nth % 12))), r)
            for j in np.flatnonzero(kind == "tie"):  # (exact under the rung's scale)
                d[j], rho = _tie(0.75 * (4 + nth[j] % 57), scales[j], proj["z_near"])
                r[j] = rho * scales[j]
                x[j], y[j] = (2 * u[j] - 1) * 0.25 * d[j] / proj["p00"], (1 - 2 * v[j]) * 0.25 * d[j] / proj["p11"]
        out = np.stack([x, y, -d, r], axis=1)
        for j in np.flatnonzero(kind == "poison"):
            c, val = _POISON[nth[j] % len(_POISON)]
            out[j, c] = -out[j, c] if val == "negate" else val
        return out

    first = n - n_c
    order = rng.permutation(first)
    lad_e, hostile, carriers = order[:n_e], order[n_e:n_e + n_h], np.arange(first, n)
    ents, mi, ml = scene.entities["model_matrix"], scene.mesh_infos, scene.meshlets
    is_rung = np.zeros(len(ml), bool)

    # the entity ladder: mesh e belongs to entity e alone (make_scene's default)
    e_scales = [float(sc._SCALE[e % len(sc._SCALE)]) for e in lad_e]
    for e, s, (x, y, z, r) in zip(lad_e, e_scales, rungs(n_e, _E_TABLE, e_scales)):
        M = np.diag([s, s, s, 1.0])
        M[:3, 3] = eye + (x, y, z)
        ents[e] = sc.mat4_cols(M.astype(F))
        mi["bounding_sphere"][e] = (0.0, 0.0, 0.0, r / s)
    # the carriers and their rungs
    for e in carriers:
        # (tall orthographic pyramids: a rung of negative radius -r passes the cone test only under a scale above r - 1)
        s = float(((16.0, 32.0, 48.0, 64.0) if tall_ortho else (1.0, 0.5, 2.0, 3.0))[e % 4])
        M = np.diag([s, s, s, 1.0])
        M[:3, 3] = eye
        ents[e] = sc.mat4_cols(M.astype(F))
        mi["bounding_sphere"][e] = (0.0, 0.0, 0.0, 1e6)
        for lod, (off, cnt) in enumerate(mi["mesh_lods"][e, :int(mi["lod_count"][e])]):
            sl = slice(int(off), int(off + cnt))
            is_rung[sl] = True
            if lod:  # never selected (the LOD target is inside the carrier's sphere: distance 0): cleared
                ml[sl] = np.zeros((), L.MESHLET)
                continue
            ml["bounding_sphere"][sl] = (rungs(int(cnt), _M_TABLE, s) / s).astype(F)
            ml["cone_cutoff"][sl] = 127  # never cone-culled: every rung reaches the HiZ test
            ml["cone_axis"][sl] = (0, 0, 127)
    # hostile entities
    kinds = ["proj_x", "proj_w", "proj_y", "t_inf", "t_nan", "t_ninf", "zero", "negative", "1e30", "1e-30", "big50",
             "big300", "neg_big"]
    factor = {"zero": 0.0, "negative": -1.0, "1e30": 1e30, "1e-30": 1e-30, "big50": 50.0, "big300": 300.0, "neg_big": -80.0}
    for e, kind in zip(hostile, _cycle(kinds, n_h)):
        m = ents[e]
        if kind == "proj_x":
            m[3] = 0.001
        elif kind == "proj_w":
            m[15] = 2.0
        elif kind == "proj_y":
            m[7] = -0.002
        elif kind in ("t_inf", "t_nan", "t_ninf"):
            m[12 + e % 3] = dict(t_inf=np.inf, t_nan=np.nan, t_ninf=-np.inf)[kind]
        else:
            with np.errstate(over="ignore"):
                m[:12] = m[:12] * F(factor[kind])
    # hostile spheres over what is no rung
    free = np.flatnonzero(~is_rung)
    pick = free[rng.random(len(free)) < 0.15]
    for j, (c, val) in zip(pick, _cycle(_sphere_kinds(), len(pick))):
        ml["bounding_sphere"][j, c] = val
    rest = np.setdiff1d(np.arange(first), lad_e)
    pick = rest[rng.random(len(rest)) < 0.35]
    for e, (c, val) in zip(pick, _cycle(_sphere_kinds(), len(pick))):
        mi["bounding_sphere"][e, c] = val
    scene.meta.update(pyramid=pyramid, ortho=ortho, ladder_entities=lad_e, carriers=carriers, hostile=hostile)
    return scene


def camera():
    """scenes.default_camera (90 degrees, 16 : 9, at (0, 2, 0), unrotated) from exact constants: no tan()."""
    proj = np.zeros((4, 4), F)
    proj[0, 0], proj[1, 1], proj[3, 2], proj[2, 3] = 0.5625, 1.0, -1.0, 0.01
    return sc.Camera(sc.translation(0.0, -2.0, 0.0), proj, float(np.pi / 2), 16.0 / 9.0, 0.01)


# ----------------------------------------------------------------------------------------------------------- census
def census(detail):
    """{class: rows} over the rows of a stage that reach the occlusion test (np_restatement's `detail` of entity_cull or
    meshlet_cull).  Everything past `not_cullable` is counted over the rows that go on to sample the pyramid."""
    reached = detail["reached"]
    cullable = detail["cullable"]
    s = reached & cullable
    g = lambda k: np.asarray(detail[k])[s]  # noqa: E731
    u, v, lod, closest, sampled, level = g("u"), g("v"), g("lod"), g("closest"), g("sampled"), g("level")
    fx, fy, w, h, vis = g("fx"), g("fy"), g("w"), g("h"), g("visible")
    mips = int(detail["mips"])
    with np.errstate(all="ignore"):
        c = {
            "not_cullable": int((reached & ~cullable).sum()),
            # z == fma(radius, scale, z_near) exactly, on a row that `>` instead of `>=` would decide the other way
            "cullable_tie_decides": int((g("cullable_tie") & ~vis).sum()),
            "uv_nan": int((np.isnan(u) | np.isnan(v)).sum()),
            "uv_outside": int(((u < 0) | (u > 1) | (v < 0) | (v > 1)).sum()),
            "lod_nan": int(np.isnan(lod).sum()),
            "lod_ninf": int((lod == -np.inf).sum()),
            "lod_negative": int((np.isfinite(lod) & (lod < 0)).sum()),
            "lod_above_top": int((lod > mips - 1).sum()),
            "lod_pinf": int((lod == np.inf).sum()),
            "clamp_left": int((fx < 0).sum()),
            "clamp_right": int((fx + 1 > w - 1).sum()),
            "clamp_top": int((fy < 0).sum()),
            "clamp_bottom": int((fy + 1 > h - 1).sum()),
            "sampled_nan": int(np.isnan(sampled).sum()),
            "sampled_pinf": int((sampled == np.inf).sum()),
            "sampled_ninf": int((sampled == -np.inf).sum()),
            "sampled_negative": int((np.isfinite(sampled) & (sampled < 0)).sum()),
            "closest_nan": int(np.isnan(closest).sum()),
            "closest_inf": int(np.isinf(closest).sum()),
        }
        for k in range(mips):
            c[f"level_{k}"] = int((level == k).sum())
        fin = np.isfinite(u) & np.isfinite(v) & np.isfinite(lod) & np.isfinite(closest) & np.isfinite(sampled)
        c["finite_visible"], c["finite_culled"] = int((fin & vis).sum()), int((fin & ~vis).sum())
        # culled by a finite texel of a level one of whose sides has collapsed to 1 (max(dim >> level, 1)): any lower
        # sample, such as a stray one, turns the row visible
        c["collapsed_level_culls"] = int((fin & ~vis & (np.minimum(w, h) == 1) & (np.maximum(w, h) > 1)).sum())
    return c


def unreachable(case):
    """{class: reason} of the classes this case cannot show."""
    out = {"lod_pinf": IMPOSSIBLE["lod_pinf"]}
    if case["ortho"]:
        for k in ("not_cullable", "cullable_tie_decides", "uv_outside", "lod_above_top"):
            out[k] = IMPOSSIBLE[k + "@ortho"]
    else:
        for k in ("closest_inf", "closest_nan"):
            out[k] = IMPOSSIBLE[k + "@persp"]
    pyr = case["pyr"]
    if len(pyr) == 1 and not case["ortho"]:
        out["cullable_tie_decides"] = IMPOSSIBLE["cullable_tie_decides@1x1"]
    with np.errstate(all="ignore"):
        has = dict(sampled_nan=np.isnan(pyr).any(), sampled_pinf=(pyr == np.inf).any(),
                   sampled_ninf=(pyr == -np.inf).any(), sampled_negative=(np.isfinite(pyr) & (pyr < 0)).any())
    if not case["floor"]:
        out["collapsed_level_culls"] = IMPOSSIBLE["collapsed_level_culls@hostile"]
    for k, present in has.items():
        if not present:
            out[k] = "the pyramid holds no such texel (it is too small for the planted blocks)"
    return out


# ------------------------------------------------------------------------------------------------------ the case set
# name -> pyramid, projection, seed, entities.  The pyramid's screen is screen_of(pyramid).  "v_*" are the committed
# reference-binary cases (tests/golden/spirv_cull_hiz_edges.npz: small, so the file stays under 1 MB).
PYRAMIDS = [(256, 128), (256, 16), (16, 256), (2, 128), (1, 1), (4096, 32), (1024, 1024)]
CASES = {}
for _k, (_w, _h) in enumerate(PYRAMIDS):
    for _o in (False, True):
        CASES[f"{'ortho' if _o else 'persp'}_{_w}x{_h}"] = dict(pyramid=(_w, _h), ortho=_o, seed=101 + 2 * _k + _o, n=500)
for _w, _h, _s in ((256, 16, 141), (16, 256, 143)):  # the tame counterparts: hostile geometry, a depth buffer with a floor
    for _o in (False, True):
        CASES[f"{'ortho' if _o else 'persp'}_{_w}x{_h}_floor"] = dict(pyramid=(_w, _h), ortho=_o, seed=_s + _o, n=500, floor=True)
VECTOR_CASES = {
    "v_persp_256x128": dict(pyramid=(256, 128), ortho=False, seed=131, n=400),
    "v_ortho_256x16": dict(pyramid=(256, 16), ortho=True, seed=132, n=400),
    "v_persp_16x256": dict(pyramid=(16, 256), ortho=False, seed=133, n=400),
    "v_ortho_1x1": dict(pyramid=(1, 1), ortho=True, seed=136, n=400),
}
_VECTOR_KW = dict(meshlets_per_mesh=((1, 8), (24, 40)), lods=2, fractions=(0.5, 0.25, 0.15))
_cache = {}


def make_case(name, oracle):
    """-> dict(scene, ci (pass 2, no planes), cam, depth, screen, pyr (the oracle's packed chain), psize, mips, ortho);
    built once per process and shared: nobody writes into it."""
    if name in _cache:
        return _cache[name]
    spec = CASES.get(name) or VECTOR_CASES[name]
    w0, h0 = spec["pyramid"]
    W, H = (1920, 1080) if (w0, h0) == (1024, 1024) else screen_of(w0, h0)
    cam = camera()
    kw = _VECTOR_KW if name in VECTOR_CASES else {}
    scene = hostile_scene(spec["seed"], spec["n"], (w0, h0), spec["ortho"], cam, **kw)
    depth = hostile_depth(spec["seed"], W, H, cam, ortho=spec["ortho"], floor=spec.get("floor", False))
    pyr, d = oracle.depth_reduce(depth, W, H)
    assert (d.width, d.height) == (w0, h0), (d.width, d.height)
    c = dict(name=name, scene=scene, cam=cam, depth=depth, screen=(W, H), pyr=pyr, psize=(w0, h0), mips=int(d.mip_levels),
             ortho=spec["ortho"], floor=spec.get("floor", False), desc=d, ci=cull_info(cam, spec["ortho"], np.zeros((0, 4), F)))
    _cache[name] = c
    return c


def cull_info(cam, ortho, planes, **kw):
    proj = ORTHO if ortho else dict(p00=cam.p00, p11=cam.p11, z_near=cam.z_near)
    return sc.make_cull_info(cam.view, planes, occlusion_pass=2, projection_type=1 if ortho else 0, **proj, **kw)


def words(scene, how, seed=0):
    """(entity, meshlet) visibility words: all zero, or random."""
    ne, nm = (scene.entity_draw_count + 31) // 32, scene.vis_words
    if how == "zero":
        return np.zeros(ne, np.uint32), np.zeros(nm, np.uint32)
    rng = np.random.default_rng(1000 + seed)
    return rng.integers(0, 2 ** 32, ne, dtype=np.uint32), rng.integers(0, 2 ** 32, nm, dtype=np.uint32)


def take_census(case, evis=None, mvis=None, ci=None):
    """-> (entity-stage census, meshlet-stage census, records, commands) of the numpy restatement on a case."""
    s = case["scene"]
    ci = case["ci"] if ci is None else ci
    if evis is None:
        evis, mvis = words(s, "zero")
    de, dm = {}, {}
    _, _, recs, _ = npr.entity_cull(ci, s.entity_draws, s.entity_draw_count, s.entity_draw_count, s.mesh_infos,
                                    s.entities, evis, case["pyr"], case["psize"], detail=de)
    cmds, _ = npr.meshlet_cull(ci, recs, s.meshlets, s.entities, s.materials, mvis, case["pyr"], case["psize"], detail=dm)
    return census(de), census(dm), recs, cmds
