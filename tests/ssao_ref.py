"""An independent numpy restatement of orbit_ssao (include/orbit_abi_ext.h A1-A9), written from shaders/ssao/ssao.comp,
ssao_blur.comp and the rules, vectorised over the pixels; it does not go through the C++ mirror.  With F = float32 every
operation is rounded on its own (numpy never contracts) and the sine and cosine are H6's polynomials restated here: the
result is what the mirror must give, byte for byte.  With F = float64 it is the GLSL evaluated in double precision with the
true sin / cos: the yardstick of tools/count_ssao.py."""
import numpy as np

PI = 3.14159265359


def _gmax(x, y):  # GLSL max as the rules have it: x < y ? y : x
    return np.where(x < y, y, x)


def _gmin(x, y):
    return np.where(y < x, y, x)


def _clamp01(x, F):
    return _gmin(_gmax(x, F(0.0)), F(1.0))


def _index(t, n):  # an integer-valued float clamped to [0, n - 1]; NaN -> 0
    t = np.where(np.isnan(t), 0.0, t)
    return np.clip(t, 0, n - 1).astype(np.int64)


def _axis(u, n, F):  # B3 of one axis
    s = u * F(n) - F(0.5)
    fl = np.floor(s)
    return _index(fl, n), _index(fl + F(1.0), n), s - fl


def sample(plane, u, v, F):
    """B3's LinearClamp sample of plane (h, w) at (u, v)."""
    h, w = plane.shape
    x0, x1, fx = _axis(u, w, F)
    y0, y1, fy = _axis(v, h, F)
    gx, gy = F(1.0) - fx, F(1.0) - fy
    return (plane[y0, x0] * gx + plane[y0, x1] * fx) * gy + (plane[y1, x0] * gx + plane[y1, x1] * fx) * fy


def project(M, x, y, z, w):
    """M x (x, y, z, w), M column-major, the sums left to right -> four arrays"""
    return [((M[r] * x + M[4 + r] * y) + M[8 + r] * z) + M[12 + r] * w for r in range(4)]


def cross(a, b):
    return [a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]]


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def normalize(v):
    n = np.sqrt(dot(v, v))
    return [c / n for c in v]


def sincos(theta, F):
    """H6's sine and cosine in float32; the true ones in float64"""
    if F is np.float64:
        return np.sin(theta), np.cos(theta)
    f = np.float32
    k = (theta * f(0.636619772) + f(0.5)).astype(np.int32)
    kf = k.astype(f)
    r = (theta - kf * f(1.5703125)) - kf * f(4.83826794897e-4)
    w = r * r
    sin_r = ((((f(-1.9515295891e-4) * w + f(8.3321608736e-3)) * w) + f(-1.6666654611e-1)) * w) * r + r
    cos_r = ((((f(2.443315711809948e-5) * w + f(-1.388731625493765e-3)) * w) + f(4.166664568298827e-2)) * w) * w + (f(1.0) - f(0.5) * w)
    q = k & 3
    s = np.select([q == 0, q == 1, q == 2], [sin_r, cos_r, -sin_r], -cos_r)
    c = np.select([q == 0, q == 1, q == 2], [cos_r, -sin_r, -cos_r], sin_r)
    return s, c


def table(samples, sample_count, min_radius, max_radius, F=np.float32):
    """A4 -> (sample_count, 4): direction, radius"""
    samples = np.asarray(samples, np.uint8)
    m = samples.shape[0]
    i = np.arange(sample_count, dtype=np.uint32)
    fi = i.astype(F) / F(sample_count)
    texel = np.floor(fi * F(m)).astype(np.int64) % m
    z = samples[texel, 2].astype(F) / F(255.0)
    bits = []
    for k in range(sample_count):  # hammersley_2d's bit reversal
        b = ((k << 16) | (k >> 16)) & 0xFFFFFFFF
        b = ((b & 0x55555555) << 1) | ((b & 0xAAAAAAAA) >> 1)
        b = ((b & 0x33333333) << 2) | ((b & 0xCCCCCCCC) >> 2)
        b = ((b & 0x0F0F0F0F) << 4) | ((b & 0xF0F0F0F0) >> 4)
        b = ((b & 0x00FF00FF) << 8) | ((b & 0xFF00FF00) >> 8)
        bits.append(b)
    rdi = np.array(bits, np.uint32).astype(F) * F(2.3283064365386963e-10)
    phi = (rdi * F(2.0)) * F(PI)
    cos_t = F(1.0) - fi
    sin_t = np.sqrt(F(1.0) - cos_t * cos_t)
    s, c = sincos(phi, F)
    zz = z * z
    radius = F(min_radius) * (F(1.0) - zz) + F(max_radius) * zz
    return np.stack([c * sin_t, s * sin_t, cos_t, radius], -1).astype(F)


def byte(c, F):
    """A6 -> (bytes uint8, nonfinite bool)"""
    nan = np.isnan(c)
    v = _clamp01(np.where(nan, F(0.0), c), F) * F(255.0) + F(0.5)
    return np.where(nan, 0, v.astype(np.int64)).astype(np.uint8), nan


def raw_pass(depth, projection, inverse_projection, noise, samples, ssao_w, ssao_h, sample_count, min_radius, max_radius, F=np.float32):
    """A1-A6 -> dict(raw (ssao_h, ssao_w) uint8, nonfinite (the same shape) bool, in_range: per-pixel counts, branch: A2's
    branch per pixel 0..3, range_inside: samples whose range_check lies strictly inside (0, 1), occluded: in-range samples
    with sample_depth >= proj.z)"""
    dep = np.asarray(depth, np.float32).astype(F)
    sh, sw = dep.shape
    P, IP = np.asarray(projection, np.float32).astype(F).reshape(16), np.asarray(inverse_projection, np.float32).astype(F).reshape(16)
    noise, ns = np.asarray(noise, np.int8), np.asarray(noise).shape[0]
    with np.errstate(all="ignore"):
        # A1: the bordered grid, pixel -1 being the shader's 0xFFFFFFFF
        px = (np.arange(-1, ssao_w + 1, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)
        py = (np.arange(-1, ssao_h + 1, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)
        u = np.broadcast_to(((px.astype(F) + F(0.5)) * (F(1.0) / F(ssao_w)))[None, :], (ssao_h + 2, ssao_w + 2))
        v = np.broadcast_to(((py.astype(F) + F(0.5)) * (F(1.0) / F(ssao_h)))[:, None], (ssao_h + 2, ssao_w + 2))
        z = sample(dep, u, v, F)
        c = project(IP, u * F(2.0) - F(1.0), (F(1.0) - v) * F(2.0) - F(1.0), z, F(1.0))
        pos = [c[k] / c[3] for k in range(3)]
        at = lambda dx, dy: [p[1 + dy:1 + dy + ssao_h, 1 + dx:1 + dx + ssao_w] for p in pos]  # noqa: E731
        p0, right, left, down, up = at(0, 0), at(1, 0), at(-1, 0), at(0, 1), at(0, -1)
        # A2
        take_right = np.abs(right[2] - p0[2]) < np.abs(left[2] - p0[2])
        take_down = np.abs(down[2] - p0[2]) < np.abs(up[2] - p0[2])
        conds = [take_right & ~take_down, take_right & take_down, ~take_right & ~take_down]
        p1 = [np.select(conds, [right[k], down[k], up[k]], left[k]) for k in range(3)]
        p2 = [np.select(conds, [up[k], right[k], left[k]], down[k]) for k in range(3)]
        normal = normalize(cross([p2[k] - p0[k] for k in range(3)], [p1[k] - p0[k] for k in range(3)]))
        branch = np.where(take_right, 0, 2) + np.where(take_down, 1, 0)
        # A3
        gx, gy = np.arange(ssao_w, dtype=np.uint32), np.arange(ssao_h, dtype=np.uint32)
        tx = np.floor((gx.astype(F) / F(ns)) * F(ns)).astype(np.int64) % ns
        ty = np.floor((gy.astype(F) / F(ns)) * F(ns)).astype(np.int64) % ns
        texel = noise[ty[:, None], tx[None, :]].astype(F)
        n = _gmax(texel / F(127.0), F(-1.0))
        rv = normalize([n[..., 0], n[..., 1], np.zeros((ssao_h, ssao_w), F)])
        d = dot(rv, normal)
        tangent = normalize([rv[k] - normal[k] * d for k in range(3)])
        bitangent = cross(normal, tangent)
        # A4, A5
        tab = table(samples, sample_count, min_radius, max_radius, F)
        occlusion = np.zeros((ssao_h, ssao_w), F)
        in_range = np.zeros((ssao_h, ssao_w), np.int64)
        range_inside = occluded_n = 0
        for i in range(sample_count):
            e = tab[i]
            sp = [p0[k] - ((tangent[k] * e[0] + bitangent[k] * e[1]) + normal[k] * e[2]) * e[3] for k in range(3)]
            c = project(P, sp[0], sp[1], sp[2], F(1.0))
            q = [c[k] / c[3] for k in range(3)]
            q[0], q[1] = q[0] * F(0.5) + F(0.5), q[1] * F(-0.5) + F(0.5)
            ok = (q[0] == _clamp01(q[0], F)) & (q[1] == _clamp01(q[1], F)) & (q[2] == _clamp01(q[2], F))
            sd = sample(dep, np.where(ok, q[0], F(0.0)), np.where(ok, q[1], F(0.0)), F)
            sdl = F(0.01) / sd
            x = F(min_radius) / np.abs(sdl - c[3])
            t = _clamp01((x - F(0.0)) / (F(1.0) - F(0.0)), F)
            rc = (t * t) * (F(3.0) - F(2.0) * t)
            occ = sd >= q[2]
            occlusion = np.where(ok, occlusion + np.where(occ, F(1.0), F(0.0)) * rc, occlusion)
            in_range += ok
            range_inside += int((ok & (rc > 0) & (rc < 1)).sum())
            occluded_n += int((ok & occ).sum())
        raw, nonfinite = byte(F(1.0) - occlusion / F(sample_count), F)
    return dict(raw=raw, nonfinite=nonfinite, in_range=in_range, branch=branch, range_inside=range_inside, occluded=occluded_n)


def blur(raw, F=np.float32):
    """A7 of raw (h, w) uint8 -> (h, w) uint8"""
    h, w = raw.shape
    t = raw.astype(F) / F(255.0)
    x, y = np.meshgrid(np.arange(w, dtype=np.uint32).astype(F), np.arange(h, dtype=np.uint32).astype(F))
    sums = []
    with np.errstate(all="ignore"):
        for ox, oy in ((0.0, 0.0), (2.0, 0.0), (0.0, 2.0), (2.0, 2.0)):
            i0, i1, _ = _axis(((x + F(0.5)) - F(ox)) / F(w), w, F)
            j0, j1, _ = _axis(((y + F(0.5)) - F(oy)) / F(h), h, F)
            sums.append(((t[j1, i0] + t[j1, i1]) + t[j0, i1]) + t[j0, i0])
        total = (((sums[0] + sums[1]) + sums[2]) + sums[3]) * F(0.0625)
    return byte(total, F)[0]


def pixel_read(blurred, screen_w, screen_h, F=np.float32):
    """A8 of blurred (h, w) uint8 -> (screen_h, screen_w) F"""
    t = blurred.astype(F) / F(255.0)
    x, y = np.meshgrid(np.arange(screen_w, dtype=np.uint32).astype(F), np.arange(screen_h, dtype=np.uint32).astype(F))
    with np.errstate(all="ignore"):
        return sample(t, (x + F(0.5)) / F(screen_w), (y + F(0.5)) / F(screen_h), F)


def ssao(depth, projection, inverse_projection, noise, samples, ssao_w=None, ssao_h=None, sample_count=32, min_radius=0.1, max_radius=0.5,
         F=np.float32):
    """The whole call -> dict(raw, blurred, ao_pixel, stats: dict of A9's four counters, and raw_pass' census arrays)"""
    sh, sw = np.asarray(depth).shape
    ssao_w, ssao_h = sw if ssao_w is None else ssao_w, sh if ssao_h is None else ssao_h
    r = raw_pass(depth, projection, inverse_projection, noise, samples, ssao_w, ssao_h, sample_count, min_radius, max_radius, F)
    blurred = blur(r["raw"], F)
    stats = dict(pixels=ssao_w * ssao_h, nonfinite_pixels=int(r["nonfinite"].sum()), unoccluded_pixels=int((r["raw"] == 255).sum()),
                 samples_in_range=int(r["in_range"].sum()))
    return dict(r, blurred=blurred, ao_pixel=pixel_read(blurred, sw, sh, F), stats=stats)
