"""An independent numpy restatement of orbit_env_map and orbit_env_sample (include/orbit_abi_ext.h E0-E12), written from
shaders/env_map/*.frag, shaders/utils/brdf_integration.frag, shaders/include/functions.glsl, src/passes/env_map_loader.rs
and the rules, vectorised over the texels; it does not go through the C++ mirror and shares nothing with
orbit_amd/csrc/env_common.h.  Where the mirror folds a tap over a cube edge in integers, this file builds a bordered copy
of every face whose border texels are found geometrically: the tap's point on the extended face plane, re-projected on
the face it falls on, in float64.  With T = float32 every operation is rounded on its own (numpy never contracts) and the
project's routines (sine / cosine, atan2c, asinc, log2c, powc) are restated here: the result is what the mirror must give,
byte for byte.  With T = float64 it is the GLSL evaluated in double precision with the true functions and exact fp16
storage: the yardstick of tools/count_env_map.py."""
import numpy as np

from post_chain_ref import log2c as _log2c32
from post_chain_ref import powc as _powc32
from ssao_ref import sincos as _sincos

F, D = np.float32, np.float64
PI = 3.14159265359
EPSILON = 0.0001
# env_map_loader.rs:109-116: (centre, up) of look_at_rh per layer
VIEWS = [((1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, 1, 0)), ((0, -1, 0), (0, 0, 1)), ((0, 1, 0), (0, 0, -1)), ((0, 0, 1), (0, 1, 0)),
         ((0, 0, -1), (0, 1, 0))]


def gmax(x, y):
    return np.where(x < y, y, x)


def gmin(x, y):
    return np.where(y < x, y, x)


def clamp(x, lo, hi):
    return gmin(gmax(x, lo), hi)


def cross(a, b):
    return [a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]]


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def normalize(v):
    with np.errstate(all="ignore"):
        n = np.sqrt(dot(v, v))
        return [c / n for c in v]


def sincos(theta, T):
    return _sincos(np.asarray(theta, T), T)


def log2(x, T):
    x = np.asarray(x, T)
    with np.errstate(all="ignore"):
        if T is D:
            return np.log2(x)
        return np.where(np.isnan(x), x, np.where(x == 0, F(-np.inf), _log2c32(np.where(x > 0, x, F(1.0))))).astype(F)


def pow5(x, T):
    if T is D:
        return np.where(x > 0, np.power(np.where(x > 0, x, 1.0), 5.0), 0.0)
    return _powc32(x, 5.0)


def atan2(y, x, T):
    """GLSL atan(y, x): E2's routine in float32, the true one in float64"""
    if T is D:
        return np.arctan2(y, x)
    f = F
    with np.errstate(all="ignore"):
        q = np.abs(y) / np.abs(x)
        big, mid = q > f(2.414213562373095), q > f(0.4142135623730950)
        y0 = np.where(big, f(1.5707963267948966), np.where(mid, f(0.7853981633974483), f(0.0))).astype(f)
        t = np.where(big, f(-1.0) / q, np.where(mid, (q - f(1.0)) / (q + f(1.0)), q)).astype(f)
        z = t * t
        p = ((((f(8.05374449538e-2) * z - f(1.38776856032e-1)) * z + f(1.99777106478e-1)) * z - f(3.33329491539e-1)) * z) * t + t
        r = y0 + p
        r = np.where(x < 0, f(PI) - r, r)
        r = np.where(y < 0, -r, r)
    return np.where((y == 0) & (x == 0), f(0.0), r).astype(f)


def asin(x, T):
    if T is D:
        with np.errstate(all="ignore"):
            return np.arcsin(x)
    f = F
    with np.errstate(all="ignore"):
        a = np.abs(x)
        big = a > f(0.5)
        z = np.where(big, f(0.5) * (f(1.0) - a), a * a).astype(f)
        t = np.where(big, np.sqrt(z), a).astype(f)
        r = (((((f(4.2163199048e-2) * z + f(2.4181311049e-2)) * z + f(4.5470025998e-2)) * z + f(7.4953002686e-2)) * z + f(1.6666752422e-1)) * z) * t + t
        r = np.where(big, f(1.5707963267948966) - (r + r), r)
        r = np.where(x < 0, -r, r)
    return np.where(a <= 1, r, f(np.nan)).astype(f)


# ---- E0
def to_half(x):
    """fp32 / fp64 values -> (np.float16 array, mask of the non-finite ones): round to nearest even, +-65504 beyond the range,
    +0 for what is not finite"""
    x = np.asarray(x)
    bad = ~np.isfinite(x)
    with np.errstate(all="ignore"):
        h = np.clip(np.where(bad, 0.0, x), -65504.0, 65504.0).astype(np.float16)
    return h, bad


def store_rgb(rgb):
    """rgb (..., 3) -> texels (..., 4) uint16 with alpha 1, and how many texels had a non-finite channel"""
    h, bad = to_half(rgb)
    out = np.empty(h.shape[:-1] + (4,), np.float16)
    out[..., :3], out[..., 3] = h, np.float16(1.0)
    return out.view(np.uint16), int(bad.any(-1).sum())


def level_size(size, m):
    return max(1, size >> m)


def layout(size, levels):
    sizes = [level_size(size, m) for m in range(levels)]
    offsets = np.concatenate([[0], np.cumsum([6 * n * n for n in sizes])]).astype(np.int64)
    return sizes, offsets


def split_levels(words, size, levels):
    """a cube in E0's layout (uint16) -> [level m as (6, n, n, 4) uint16]"""
    sizes, offsets = layout(size, levels)
    w = np.asarray(words, np.uint16).reshape(-1, 4)
    assert len(w) == offsets[-1]
    return [w[offsets[m]:offsets[m + 1]].reshape(6, n, n, 4) for m, n in enumerate(sizes)]


# ---- E1, from the loader: look_at_rh, transposed, applied to (cx, cy, 1)
def look_at_rh(center, up):
    f = np.asarray(center, D) / np.linalg.norm(center)
    s = np.cross(f, np.asarray(up, D))
    s = s / np.linalg.norm(s)
    u = np.cross(s, f)
    return np.stack([s, u, -f])  # the rotation's rows; the eye is the origin


def local_pos(face, n, T):
    """in_local_pos of every texel of a layer n texels wide -> three (n, n) arrays [py, px].  transpose(V) has one entry of
    +-1 per row: the product is that component, negated or not (a product with the zeros would lose the sign of a zero)"""
    V = look_at_rh(*VIEWS[face])
    px = np.arange(n).astype(T)
    cx = (T(2.0) * (px + T(0.5))) / T(n) - T(1.0)
    cy = T(1.0) - (T(2.0) * (px + T(0.5))) / T(n)
    comps = [np.broadcast_to(cx[None, :], (n, n)), np.broadcast_to(cy[:, None], (n, n)), np.ones((n, n), T)]
    out = []
    for k in range(3):
        col = V[:, k]  # row k of the transpose
        (idx,) = np.nonzero(np.round(col))
        assert len(idx) == 1 and abs(abs(col[idx[0]]) - 1) < 1e-12
        out.append(comps[idx[0]].astype(T) if col[idx[0]] > 0 else -comps[idx[0]].astype(T))
    return out


# ---- E2
def equirect_level(pano, n, T):
    """equirectangular_cube_map.frag over the six layers -> rgb (6, n, n, 3) in T"""
    pano = np.asarray(pano, T)
    h, w = pano.shape[:2]
    out = np.empty((6, n, n, 3), T)
    for face in range(6):
        v = normalize(local_pos(face, n, T))
        ux = atan2(v[2], v[0], T) * T(0.1591) + T(0.5)
        uy = T(1.0) - (asin(v[1], T) * T(0.3183) + T(0.5))
        sx, sy = ux * T(w) - T(0.5), uy * T(h) - T(0.5)
        flx, fly = np.floor(sx), np.floor(sy)
        fx, fy = (sx - flx)[..., None], (sy - fly)[..., None]
        x0, y0 = flx.astype(np.int64) % w, fly.astype(np.int64) % h
        x1, y1 = (flx.astype(np.int64) + 1) % w, (fly.astype(np.int64) + 1) % h
        gx, gy = T(1.0) - fx, T(1.0) - fy
        with np.errstate(all="ignore"):
            c = (pano[y0, x0, :3] * gx + pano[y0, x1, :3] * fx) * gy + (pano[y1, x0, :3] * gx + pano[y1, x1, :3] * fx) * fy
            out[face] = clamp(c, T(0.0), T(10000.0))
    return out


# ---- E3
def mip_level(texels, T):
    """(6, 2n, 2n, 4) uint16 -> the level below as floats (6, n, n, 4)"""
    t = texels.view(np.float16).astype(T)
    return ((t[:, 0::2, 0::2] + t[:, 0::2, 1::2]) + (t[:, 1::2, 0::2] + t[:, 1::2, 1::2])) * T(0.25)


def sky_cube(pano, size, T):
    """-> (words uint16 (sky_texels * 4,), texels with a non-finite channel)"""
    levels = size.bit_length()
    lv, bad = store_rgb(equirect_level(pano, size, T))
    out = [lv]
    for _ in range(1, levels):
        h, b = to_half(mip_level(out[-1], T))
        out.append(h.view(np.uint16))
        bad += int(b.any(-1).sum())
    return np.concatenate([o.reshape(-1) for o in out]), bad


# ---- E4
def face_select(d):
    """Vulkan's table -> layer, sc, tc, ma"""
    x, y, z = d
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    zmaj = (az >= ax) & (az >= ay)
    ymaj = ~zmaj & (ay >= ax)
    face = np.where(zmaj, np.where(z < 0, 5, 4), np.where(ymaj, np.where(y < 0, 3, 2), np.where(x < 0, 1, 0)))
    sc = np.where(zmaj, np.where(z < 0, -x, x), np.where(ymaj, x, np.where(x < 0, z, -z)))
    tc = np.where(zmaj, -y, np.where(ymaj, np.where(y < 0, -z, z), -y))
    ma = np.where(zmaj, az, np.where(ymaj, ay, ax))
    return face, sc, tc, ma


def face_point(face, sc, tc):
    """the point of layer `face`'s plane at (sc, tc), ma = 1: the table read backwards"""
    return [(1.0, -tc, -sc), (-1.0, -tc, sc), (sc, 1.0, tc), (sc, -1.0, -tc), (sc, -tc, 1.0), (-sc, -tc, -1.0)][face]


def neighbour(face, i, j, n):
    """the texel a tap at (i, j) of `face` lands on, one of i, j outside 0 .. n - 1: geometrically, in float64"""
    p = face_point(face, (2 * i + 1 - n) / n, (2 * j + 1 - n) / n)
    f2, sc, tc, ma = face_select([np.float64(c) for c in p])
    s, t = 0.5 * sc / ma + 0.5, 0.5 * tc / ma + 0.5
    i2, j2 = int(np.floor(s * n)), int(np.floor(t * n))
    assert int(f2) != face and 0 <= i2 < n and 0 <= j2 < n
    return int(f2), i2, j2


def bordered(level):
    """(6, n, n, 3) floats -> (6, n + 2, n + 2, 3): every face with the texels around it; a corner is the mean of the three
    texels that meet there, ((own + across x) + across y) / 3"""
    n = level.shape[1]
    T = level.dtype.type
    out = np.zeros((6, n + 2, n + 2, 3), T)
    out[:, 1:-1, 1:-1] = level
    for face in range(6):
        for k in range(n):
            for (i, j) in ((-1, k), (n, k), (k, -1), (k, n)):
                f2, i2, j2 = neighbour(face, i, j, n)
                out[face, j + 1, i + 1] = level[f2, j2, i2]
    for face in range(6):
        for (i, j) in ((-1, -1), (n, -1), (-1, n), (n, n)):
            ci, cj = min(max(i, 0), n - 1), min(max(j, 0), n - 1)
            with np.errstate(all="ignore"):
                out[face, j + 1, i + 1] = ((level[face, cj, ci] + out[face, cj + 1, i + 1]) + out[face, j + 1, ci + 1]) / T(3.0)
    return out


class Cube:
    """A stored cube (E0) as the sampler reads it"""

    def __init__(self, words, size, levels, T):
        self.T, self.size, self.levels = T, size, levels
        self.border = [bordered(lv.view(np.float16).astype(T)[..., :3]) for lv in split_levels(words, size, levels)]

    def _level(self, m, face, s, t):
        T = self.T
        b = self.border[m]
        n = b.shape[1] - 2
        x, y = s * T(n) - T(0.5), t * T(n) - T(0.5)
        flx, fly = np.floor(x), np.floor(y)
        fx, fy = (x - flx)[:, None], (y - fly)[:, None]
        i0, j0 = flx.astype(np.int64) + 1, fly.astype(np.int64) + 1
        gx, gy = T(1.0) - fx, T(1.0) - fy
        with np.errstate(all="ignore"):
            return (b[face, j0, i0] * gx + b[face, j0, i0 + 1] * fx) * gy + (b[face, j0 + 1, i0] * gx + b[face, j0 + 1, i0 + 1] * fx) * fy

    def sample(self, d, lod):
        """textureLod over directions d = [x, y, z] (arrays of one shape (N,)) and lod (N,) -> rgb (N, 3), bad (N,) bool"""
        T = self.T
        d = [np.asarray(c, T) for c in d]
        lod = np.asarray(lod, T)
        bad = ~(np.isfinite(d[0]) & np.isfinite(d[1]) & np.isfinite(d[2])) | ((d[0] == 0) & (d[1] == 0) & (d[2] == 0))
        safe = [np.where(bad, T(1.0), c) for c in d]
        face, sc, tc, ma = face_select(safe)
        s, t = (T(0.5) * sc) / ma + T(0.5), (T(0.5) * tc) / ma + T(0.5)
        with np.errstate(all="ignore"):
            lod = np.where(lod > 0, lod, T(0.0))
        lod = np.where(lod > T(self.levels - 1), T(self.levels - 1), lod).astype(T)
        lf = np.floor(lod)
        f = (lod - lf)[:, None]
        out = np.zeros(lod.shape + (3,), T)
        li = lf.astype(np.int64)
        for m in range(self.levels):
            at = (li == m) & ~bad
            if not at.any():
                continue
            a = self._level(m, face[at], s[at], t[at])
            mixed = (f[at] != 0)[:, 0]
            if mixed.any():
                b = self._level(m + 1, face[at][mixed], s[at][mixed], t[at][mixed])
                fm = f[at][mixed]
                with np.errstate(all="ignore"):
                    a[mixed] = a[mixed] * (T(1.0) - fm) + b * fm
            out[at] = a
        return out, bad


# ---- E5
def irradiance(sky, n, sample_delta, T, lod=None):
    """cubemap_convolution.frag over the six layers of an n x n cube -> rgb (6, n, n, 3), bad directions"""
    if lod is None:
        lod = gmax(T(0.0), log2(T(sky.size) / T(n), T))
    out, bad = np.empty((6, n, n, 3), T), 0
    delta = T(sample_delta)
    for face in range(6):
        p = [c.reshape(-1) for c in local_pos(face, n, T)]
        normal = normalize(p)
        up = [np.zeros_like(p[0]), np.ones_like(p[0]), np.zeros_like(p[0])]
        right = normalize(cross(up, normal))
        up = normalize(cross(normal, right))
        total, count = np.zeros((n * n, 3), T), T(0.0)
        phi = T(0.0)
        while phi < T(2.0) * T(PI):
            sp, cp = sincos(phi, T)
            theta = T(0.0)
            while theta < T(0.5) * T(PI):
                st, ct = sincos(theta, T)
                tx, ty = T(st * cp), T(st * sp)
                with np.errstate(all="ignore"):
                    vec = [(tx * right[k] + ty * up[k]) + T(ct) * p[k] for k in range(3)]
                    c, b = sky.sample(vec, np.full(n * n, lod, T))
                    total = total + (c * T(ct)) * T(st)
                bad += int(b.sum())
                count = T(count + T(1.0))
                theta = T(theta + delta)
            phi = T(phi + delta)
        with np.errstate(all="ignore"):
            out[face] = ((T(PI) * total) * (T(1.0) / count)).reshape(n, n, 3)
    return out, bad


# ---- E6
def radical_inverse(i):
    bits = np.uint32(i)
    bits = (bits << np.uint32(16)) | (bits >> np.uint32(16))
    for mask, shift in ((0x55555555, 1), (0x33333333, 2), (0x0F0F0F0F, 4), (0x00FF00FF, 8)):
        bits = ((bits & np.uint32(mask)) << np.uint32(shift)) | ((bits & np.uint32(~mask & 0xFFFFFFFF)) >> np.uint32(shift))
    return bits


def random(x, y, T):
    dt = x * T(12.9898) + y * T(78.233)
    sn = dt - T(3.14) * np.floor(dt / T(3.14))  # GLSL mod
    s, _ = sincos(sn, T)
    v = s * T(43758.5453)
    return v - np.floor(v)  # fract


def ggx_frame(normal, T, normalise_y):
    z_up = np.abs(normal[2]) < T(0.999)
    up = [np.where(z_up, T(0.0), T(1.0)), np.zeros_like(normal[0]), np.where(z_up, T(1.0), T(0.0))]
    tx = normalize(cross(up, normal))
    ty = cross(normal, tx)
    return tx, (normalize(ty) if normalise_y else ty), z_up


def distribution_ggx(ndh, roughness, T):
    a = roughness * roughness
    a2 = a * a
    den = (ndh * ndh) * (a2 - T(1.0)) + T(1.0)
    den = (T(PI) * den) * den
    return a2 / gmax(den, T(EPSILON))


def prefilter_level(sky, n, roughness, sample_count, T, census=None):
    """environmental_map_prefilter.frag over the six layers of an n x n level -> rgb (6, n, n, 3), bad directions"""
    out, bad = np.empty((6, n, n, 3), T), 0
    roughness = T(roughness)
    dim = T(sky.size)
    omega_p = (T(4.0) * T(PI)) / ((T(6.0) * dim) * dim)
    for face in range(6):
        N = normalize([c.reshape(-1) for c in local_pos(face, n, T)])
        tx, ty, z_up = ggx_frame(N, T, True)
        phase = random(N[0], N[2], T) * T(0.1)
        color, weight = np.zeros((n * n, 3), T), np.zeros(n * n, T)
        for i in range(sample_count):
            xi_x, xi_y = T(i) / T(sample_count), T(radical_inverse(i)) * T(2.3283064365386963e-10)
            alpha = roughness * roughness
            phi = (T(2.0) * T(PI)) * xi_x + phase
            cos_t = np.sqrt((T(1.0) - xi_y) / (T(1.0) + (alpha * alpha - T(1.0)) * xi_y))
            sin_t = np.sqrt(T(1.0) - cos_t * cos_t)
            s, c = sincos(phi, T)
            hx, hy = sin_t * c, sin_t * s
            H = normalize([(tx[k] * hx + ty[k] * hy) + N[k] * cos_t for k in range(3)])
            vh = dot(N, H)
            L = [(T(2.0) * vh) * H[k] - N[k] for k in range(3)]
            ndl = clamp(dot(N, L), T(0.0), T(1.0))
            on = ndl > 0
            ndh = clamp(dot(N, H), T(0.0), T(1.0))
            with np.errstate(all="ignore"):
                pdf = (distribution_ggx(ndh, roughness, T) * ndh) / (T(4.0) * ndh) + T(0.0001)
                omega_s = T(1.0) / (T(sample_count) * pdf)
                mip = np.zeros_like(ndl) if roughness == 0 else gmax(T(0.5) * log2(omega_s / omega_p, T) + T(1.0), T(0.0))
                rgb, b = sky.sample([np.where(on, L[k], T(1.0)) for k in range(3)], mip)
                color = np.where(on[:, None], color + rgb * ndl[:, None], color)
                weight = np.where(on, weight + ndl, weight)
            bad += int((b & on).sum())
            if census is not None:
                census["ndl_not_positive"] += int((~on).sum())
        with np.errstate(all="ignore"):
            out[face] = (color / weight[:, None]).reshape(n, n, 3)
        if census is not None:
            census["z_up"] += int(z_up.sum())
            census["x_up"] += int((~z_up).sum())
            census["weight_zero_texels"] += int((weight == 0).sum())
            census["roughness_zero_texels"] += n * n if roughness == 0 else 0
    return out, bad


def prefiltered_cube(sky, size, levels, sample_count, T, census=None):
    """-> (words uint16, texels with a non-finite channel, bad directions)"""
    words, nonfinite, bad = [], 0, 0
    for m in range(levels):
        roughness = T(m) / T(levels - 1) if levels > 1 else T(0.0)
        rgb, b = prefilter_level(sky, level_size(size, m), roughness, sample_count, T, census)
        w, nf = store_rgb(rgb)
        words.append(w.reshape(-1))
        nonfinite, bad = nonfinite + nf, bad + b
    return np.concatenate(words), nonfinite, bad


# ---- E7
def brdf_table(n, sample_count, T):
    """brdf_integration.frag over an n x n table -> (words uint16 (n * n * 2,), texels with a non-finite channel)"""
    c = (np.arange(n).astype(T) + T(0.5)) / T(n)
    ndv, roughness = np.broadcast_to(c[None, :], (n, n)).reshape(-1), np.broadcast_to(c[:, None], (n, n)).reshape(-1)
    zero, one = np.zeros_like(ndv), np.ones_like(ndv)
    V, N = [np.sqrt(T(1.0) - ndv * ndv), zero, ndv], [zero, zero, one]
    tangent, bitangent, _ = ggx_frame(N, T, False)

    def schlick(x):
        k = (roughness * roughness) / T(2.0)
        return x / (x * (T(1.0) - k) + k)

    A, B = np.zeros_like(ndv), np.zeros_like(ndv)
    for i in range(sample_count):
        xi_x, xi_y = T(i) / T(sample_count), T(radical_inverse(i)) * T(2.3283064365386963e-10)
        a = roughness * roughness
        phi = (T(2.0) * T(PI)) * xi_x
        with np.errstate(all="ignore"):
            cos_t = np.sqrt((T(1.0) - xi_y) / (T(1.0) + (a * a - T(1.0)) * xi_y))
            sin_t = np.sqrt(T(1.0) - cos_t * cos_t)
            s, co = sincos(phi, T)
            hx, hy = T(co) * sin_t, T(s) * sin_t
            H = normalize([(tangent[k] * hx + bitangent[k] * hy) + N[k] * cos_t for k in range(3)])
            vh = dot(V, H)
            L = normalize([(T(2.0) * vh) * H[k] - V[k] for k in range(3)])
            ndl, ndh, vdh = gmax(L[2], T(0.0)), gmax(H[2], T(0.0)), gmax(vh, T(0.0))
            G = schlick(gmax(dot(N, L), T(0.0))) * schlick(gmax(dot(N, V), T(0.0)))
            g_vis = (G * vdh) / (ndh * ndv)
            fc = pow5(T(1.0) - vdh, T)
            on = ndl > 0
            A = np.where(on, A + (T(1.0) - fc) * g_vis, A)
            B = np.where(on, B + fc * g_vis, B)
    with np.errstate(all="ignore"):
        h, bad = to_half(np.stack([A / T(sample_count), B / T(sample_count)], -1))
    return h.view(np.uint16).reshape(-1), int(bad.any(-1).sum())


# ---- the whole call
def env_map(pano=None, sky_words=None, sky_size=0, irradiance_size=0, prefiltered_size=0, prefiltered_levels=0, brdf_size=0,
            sample_count=4096, sample_delta=0.025, brdf_sample_count=1024, T=F, census=None):
    """-> dict(sky, irradiance, prefiltered, brdf: uint16 words or None; stats: dict of E8's five counters)"""
    st = dict(sky_nonfinite=0, irradiance_nonfinite=0, prefiltered_nonfinite=0, brdf_nonfinite=0, bad_directions=0)
    out = dict(sky=None, irradiance=None, prefiltered=None, brdf=None, stats=st)
    if pano is not None and sky_size:
        sky_words, st["sky_nonfinite"] = sky_cube(pano, sky_size, T)
        out["sky"] = sky_words
    sky = Cube(sky_words, sky_size, sky_size.bit_length(), T) if sky_words is not None and (irradiance_size or prefiltered_size) else None
    if irradiance_size:
        rgb, bad = irradiance(sky, irradiance_size, sample_delta, T)
        words, st["irradiance_nonfinite"] = store_rgb(rgb)
        out["irradiance"] = words.reshape(-1)
        st["bad_directions"] += bad
    if prefiltered_size:
        out["prefiltered"], st["prefiltered_nonfinite"], bad = prefiltered_cube(sky, prefiltered_size, prefiltered_levels, sample_count, T, census)
        st["bad_directions"] += bad
    if brdf_size:
        out["brdf"], st["brdf_nonfinite"] = brdf_table(brdf_size, brdf_sample_count, T)
    return out
