"""An independent numpy restatement of orbit_bloom and orbit_post_process (include/orbit_abi_ext.h B1-B9 and T1-T5), written
from the rules and the reference's GLSL, sharing nothing with orbit_amd/csrc/post_common.h: whole levels at once, every
float32 operation numpy's (each rounded on its own), the B10G11R11 encoding by frexp and floor instead of bit fields,
log2c and exp2c as the rules state them.  Every routine takes the float type: with T = float64 and pow = numpy's the same
text is the GLSL evaluated in double, with a true pow, levels still stored through B7 — what the accuracy figures are
measured against."""
import numpy as np

F = np.float32
D = np.float64
LOG2C = [float.fromhex(h) for h in ("-0x1.cebep-4", "0x1.80ab18p-3", "-0x1.865ffcp-3", "0x1.a265fcp-3", "-0x1.eac694p-3", "0x1.2782e6p-2",
                                     "-0x1.715a68p-2", "0x1.ec708p-2", "-0x1.71547p-1", "0x1.715476p+0")]
EXP2C = [1.5252734e-5, 1.5403530e-4, 1.3333558e-3, 9.6181291e-3, 5.5504109e-2, 2.4022651e-1, 6.9314718e-1, 1.0]  # ln(2)^n / n!, n = 7..0
MAX_LEVELS = 6


def log2c(x):
    """L2's log2 of positive finite float32 (subnormals included), +inf -> +inf"""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        small = x < F(2.0 ** -126)
        xs = np.where(small, x * F(16777216.0), x).astype(F)
        b = xs.view(np.uint32)
        e = (b >> np.uint32(23)).astype(np.int64) - 127 - np.where(small, 24, 0)
        m = ((b & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(F)
        big = m > F(1.41421354)
        m = np.where(big, m * F(0.5), m).astype(F)
        e = e + big
        f = m - F(1.0)
        p = np.full(x.shape, F(LOG2C[0]), F)
        for c in LOG2C[1:]:
            p = p * f
            p = p + F(c)
        out = p * f + e.astype(F)
    return np.where(np.isinf(x), F(np.inf), out).astype(F)


def exp2c(x):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        xc = np.where(np.isfinite(x), np.clip(x, F(-126.0), F(127.99999)), F(0.0)).astype(F)
        k = np.floor(xc + F(0.5))
        r = xc - k
        p = np.full(x.shape, F(EXP2C[0]), F)
        for c in EXP2C[1:]:
            p = p * r
            p = p + F(c)
        top = k > 127  # 2^128 is no float: 2^127 * (2 p)
        p = np.where(top, p * F(2.0), p).astype(F)
        out = np.ldexp(F(1.0), np.where(top, 127, k).astype(np.int32)).astype(F) * p
        out = np.where(x >= F(128.0), F(np.inf), np.where(x < F(-126.0), F(0.0), out))
    return np.where(np.isnan(x), x, out).astype(F)


def powc(x, y):
    """B5 / T4: exp2c(y * log2c(x)), 0 for x <= 0 and NaN"""
    x = np.asarray(x, F)
    pos = x > 0
    with np.errstate(all="ignore"):
        out = exp2c(F(y) * log2c(np.where(pos, x, F(1.0))))
    return np.where(pos, out, F(0.0)).astype(F)


def pow64(x, y):
    x = np.asarray(x, D)
    with np.errstate(all="ignore"):
        return np.where(x > 0, np.power(np.where(x > 0, x, 1.0), D(y)), 0.0)


# ---- B7
def encode(x, mant):
    """One component (any float type) -> (code, clamped): truncation toward zero, by frexp and floor"""
    x = np.asarray(x)
    big = D((2.0 - 2.0 ** -mant) * 2.0 ** 15)  # 65024 / 64512
    max_code = (30 << mant) | ((1 << mant) - 1)
    with np.errstate(all="ignore"):
        ok = np.isfinite(x) & (x > 0)
        v = np.where(ok, x, 1.0).astype(D)  # exact for float32
        frac, ex = np.frexp(v)  # v = frac * 2^ex, frac in [0.5, 1)
        e = ex - 1
        normal = np.floor((frac * 2.0 - 1.0) * (1 << mant)).astype(np.int64) | ((e + 15).astype(np.int64) << mant)
        tiny = np.floor(v * 2.0 ** (14 + mant)).astype(np.int64)
        code = np.where(e >= -14, normal, tiny)
        clamped = ok & (v >= big)
        code = np.where(clamped, max_code, code)
    return np.where(ok, code, 0).astype(np.uint32), clamped


def decode(code, mant):
    code = np.asarray(code, np.uint32).astype(np.int64)
    e, m = code >> mant, code & ((1 << mant) - 1)
    with np.errstate(all="ignore"):
        normal = (1.0 + m / D(1 << mant)) * np.exp2((e - 15).astype(D))
        out = np.where(e == 0, m * 2.0 ** -(14 + mant), normal)
        out = np.where(e == 31, np.where(m == 0, np.inf, np.nan), out)
    return out.astype(F)


def pack(rgb):
    """(..., 3) -> (words (...), clamped (...))"""
    rgb = np.asarray(rgb)
    r, cr = encode(rgb[..., 0], 6)
    g, cg = encode(rgb[..., 1], 6)
    b, cb = encode(rgb[..., 2], 5)
    return (r | (g << np.uint32(11)) | (b << np.uint32(22))).astype(np.uint32), cr | cg | cb


def unpack(words):
    w = np.asarray(words, np.uint32)
    return np.stack([decode(w & np.uint32(0x7FF), 6), decode((w >> np.uint32(11)) & np.uint32(0x7FF), 6), decode(w >> np.uint32(22), 5)], axis=-1)


# ---- B1, B2
def layout(width, height, max_levels=MAX_LEVELS):
    levels = min(max(1, int(np.floor(np.log2(max(width, height)))) + 1), MAX_LEVELS, max_levels)
    sizes = [(max(width >> k, 1), max(height >> k, 1)) for k in range(levels)]
    offsets = [int(sum(w * h for w, h in sizes[:k])) for k in range(levels)]
    return dict(levels=levels, sizes=sizes, offsets=offsets, total_texels=int(sum(w * h for w, h in sizes)))


def threshold_filter(threshold, soft_threshold):
    knee = F(threshold) * F(soft_threshold)
    return [F(threshold), F(threshold) - knee, F(2.0) * knee, F(0.25) / (knee + F(0.00001))]


# ---- B3
def axis(u, n, T):
    """u (k,) of type T -> i0, i1 (int64, clamped), f"""
    with np.errstate(all="ignore"):
        s = u * T(n) - T(0.5)
        fl = np.floor(s)
        f = s - fl

        def index(t):
            t = np.nan_to_num(t, nan=0.0, posinf=float(n), neginf=-1.0)
            return np.clip(t, 0, n - 1).astype(np.int64)
    return index(fl), index(fl + T(1.0)), f


def sample(src, u, v, T):
    """src (h, w, 3) of type T at the grid v (H,) x u (W,) -> (H, W, 3)"""
    h, w = src.shape[:2]
    x0, x1, fx = axis(u, w, T)
    y0, y1, fy = axis(v, h, T)
    fx, fy = fx[None, :, None], fy[:, None, None]
    gx, gy = T(1.0) - fx, T(1.0) - fy
    t00, t10 = src[y0[:, None], x0[None, :]], src[y0[:, None], x1[None, :]]
    t01, t11 = src[y1[:, None], x0[None, :]], src[y1[:, None], x1[None, :]]
    with np.errstate(all="ignore"):
        return (t00 * gx + t10 * fx) * gy + (t01 * gx + t11 * fx) * fy


# ---- B4, B5
def karis(c, T, power):
    with np.errstate(all="ignore"):
        s = power(c, T(F(1.0 / 2.2)))
        luma = ((s[..., 0] * T(F(0.2126)) + s[..., 1] * T(F(0.7152))) + s[..., 2] * T(F(0.0722))) * T(0.25)
        return (T(1.0) / (T(1.0) + luma))[..., None]


def gmax(x, y):
    return np.where(x < y, y, x)


def prefilter(c, tf, T):
    tf = [T(t) for t in tf]
    with np.errstate(all="ignore"):
        m = gmax(c[..., 0], gmax(c[..., 1], c[..., 2]))
        soft = gmax(m - tf[1], T(0.0))
        soft = np.where(tf[2] < soft, tf[2], soft)
        soft = (soft * soft) * tf[3]
        contribution = gmax(m - tf[0], soft) / gmax(m, T(F(0.00001)))
        return c * contribution[..., None]


def downsample(src, dst_w, dst_h, level0=False, tf=None, T=F, power=powc):
    """One downsample of src (h, w, 3) -> (dst_h, dst_w, 3), unpacked"""
    src = np.asarray(src, T)
    xs, ys = np.arange(dst_w).astype(T) + T(0.5), np.arange(dst_h).astype(T) + T(0.5)
    rx, ry = T(1.0) / T(dst_w), T(1.0) / T(dst_h)

    def tap(dx, dy):
        return sample(src, (xs + T(dx)) * rx, (ys + T(dy)) * ry, T)
    x = tap(0, 0)
    y0, y1, y2, y3 = tap(1, 1), tap(-1, 1), tap(1, -1), tap(-1, -1)
    z0, z1, z2, z3 = tap(-2, -2), tap(-2, 0), tap(-2, 2), tap(0, -2)
    z4, z5, z6, z7 = tap(0, 2), tap(2, -2), tap(2, 0), tap(2, 2)
    with np.errstate(all="ignore"):
        g = [(y0 + y1 + y2 + y3) * T(0.125), (z0 + z0 + z3 + x) * T(0.03125), (z1 + z2 + z4 + x) * T(0.03125),
             (z3 + z5 + z6 + x) * T(0.03125), (z4 + z6 + z7 + x) * T(0.03125)]
        if level0:
            g = [gk * karis(gk, T, power) for gk in g]
        result = g[0] + g[1] + g[2] + g[3] + g[4]
        if level0:
            result = prefilter(result, tf, T)
    return result.astype(T)


# ---- B6
def upsample_term(src, dst_w, dst_h, r, T=F):
    src = np.asarray(src, T)
    bx, by = np.arange(dst_w).astype(T) * (T(1.0) / T(dst_w)), np.arange(dst_h).astype(T) * (T(1.0) / T(dst_h))
    r = T(F(r))

    def tap(ox, oy):
        with np.errstate(all="ignore"):
            return sample(src, bx + ox, by + oy, T)
    z = T(0.0)
    x = tap(z, z)
    y0, y1, y2, y3 = tap(r, z), tap(z, r), tap(-r, z), tap(z, -r)
    z0, z1, z2, z3 = tap(r, r), tap(-r, -r), tap(-r, r), tap(r, -r)
    with np.errstate(all="ignore"):
        return (x * T(0.25) + (y0 + y1 + y2 + y3) * T(0.125) + (z0 + z1 + z2 + z3) * T(0.0625)).astype(T)


def finite_or_zero(a):
    return np.where(np.isfinite(a), a, F(0.0)).astype(F)


# ---- B1-B9
def bloom(color, threshold=0.0, soft_threshold=0.0, filter_radius=0.003, max_levels=MAX_LEVELS, T=F, power=powc):
    """color (h, w, 4) float32 -> dict(mips np.uint32 (total,), stats dict, layout)"""
    color = np.asarray(color, F)
    h, w = color.shape[:2]
    lay = layout(w, h, max_levels)
    tf = threshold_filter(threshold, soft_threshold)
    rgb = color[..., :3]
    stats = dict(levels=lay["levels"], texels_written=0, nonfinite_inputs=int((~np.isfinite(rgb)).any(axis=-1).sum()), clamped_texels=0)
    levels = []
    src = finite_or_zero(rgb)
    for k, (lw, lh) in enumerate(lay["sizes"]):
        words, clamped = pack(downsample(src.astype(T), lw, lh, k == 0, tf, T, power))
        stats["texels_written"] += lw * lh
        stats["clamped_texels"] += int(clamped.sum())
        levels.append(words)
        src = unpack(words)
    for k in range(lay["levels"] - 1, 0, -1):
        lw, lh = lay["sizes"][k - 1]
        with np.errstate(all="ignore"):
            total = unpack(levels[k - 1]).astype(T) + upsample_term(unpack(levels[k]).astype(T), lw, lh, filter_radius, T)
        words, clamped = pack(total)
        stats["texels_written"] += lw * lh
        stats["clamped_texels"] += int(clamped.sum())
        levels[k - 1] = words
    return dict(mips=np.concatenate([l.reshape(-1) for l in levels]).astype(np.uint32), stats=stats, layout=lay)


# ---- T1-T5
ACES_IN = [[0.59719, 0.07600, 0.02840], [0.35458, 0.90834, 0.13383], [0.04823, 0.01566, 0.83777]]  # columns, as the GLSL lists them
ACES_OUT = [[1.60475, -0.10208, -0.00327], [-0.53108, 1.10813, -0.07276], [-0.07367, -0.00605, 1.07602]]


def mat3(cols, v, T):
    with np.errstate(all="ignore"):
        return np.stack([(T(F(cols[0][i])) * v[..., 0] + T(F(cols[1][i])) * v[..., 1]) + T(F(cols[2][i])) * v[..., 2] for i in range(3)], axis=-1)


def post_process(color, bloom=None, exposure=1.0, bloom_intensity=0.025, render_mode=0, bgra=False, T=F, power=powc):
    """color (h, w, 4) float32, bloom: None or packed words (>= h * w) -> dict(ldr (h, w, 4), rgba8 (h, w, 4) uint8, stats dict)"""
    color = np.asarray(color, F)
    h, w = color.shape[:2]
    rgb = color[..., :3]
    bad = (~np.isfinite(rgb)).any(axis=-1)
    hdr = finite_or_zero(rgb).astype(T)
    bloomed = np.zeros((h, w), bool)
    with np.errstate(all="ignore"):
        if render_mode == 0 and bloom is not None:
            term = unpack(np.asarray(bloom, np.uint32).reshape(-1)[:h * w].reshape(h, w)).astype(T) * T(F(bloom_intensity))
            bloomed = (term != 0).any(axis=-1)
            hdr = hdr + term
            bad |= (~np.isfinite(hdr)).any(axis=-1)
            hdr = np.where(np.isfinite(hdr), hdr, T(0.0))
        v = mat3(ACES_IN, hdr * T(F(exposure)), T)
        a = v * (v + T(F(0.0245786))) - T(F(0.000090537))
        b = v * (T(F(0.983729)) * v + T(F(0.4329510))) + T(F(0.238081))
        m = mat3(ACES_OUT, a / b, T)
        m = np.where(m > 0, np.where(m < 1, m, T(1.0)), T(0.0)).astype(T)  # NaN -> 0
        srgb = np.where(m < T(F(0.0031308)), m * T(F(12.92)), T(F(1.055)) * power(m, T(F(1.0 / 2.4))) - T(F(0.055)))
        byte = (srgb.astype(T) * T(255.0) + T(0.5)).astype(np.int64).astype(np.uint8)
    ldr = np.concatenate([m, np.ones((h, w, 1), T)], axis=-1)
    order = [2, 1, 0] if bgra else [0, 1, 2]
    rgba8 = np.concatenate([byte[..., order], np.full((h, w, 1), 255, np.uint8)], axis=-1)
    return dict(ldr=ldr, rgba8=rgba8, stats=dict(pixels=h * w, nonfinite_pixels=int(bad.sum()), bloom_pixels=int(bloomed.sum())))
