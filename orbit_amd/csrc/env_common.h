// env_common.h — the arithmetic of orbit_env_map and orbit_env_sample (include/orbit_abi_ext.h E0-E12),
// written once for the device kernels (env_map.hip) and the host mirror (orbit_amd/host/orbit_env_map.cpp).  The pieces:
// env_half / env_unhalf are E0's storage; env_layout its shape; env_atan2c / env_asinc the routines E2 needs;
// env_texel_direction is E1; env_equirect_texel E2; env_mip_texel E3; env_sample E4 over an EnvCube; env_irradiance_texel
// E5; env_prefilter_entry / env_prefilter_frame / env_prefilter_sample / env_prefilter_end the sample-only, texel-only and
// per-pair parts of E6; env_brdf_texel E7; env_map_check / env_sample_check E9, for the entry points and the mirror alike.
// fp32, every operation rounded on its own.  Equal inputs, equal functions: equal bytes.
#pragma once
#include "post_common.h" // post_powc, and shade_common.h's shade_log2c / shade_max / clamp / dot / normalize, shadow_sincos

namespace orbit {
namespace raster {

constexpr uint32_t kEnvMaxLevels = ORBIT_ENV_MAX_LEVELS;

// ---- E0: fp16 storage
// fp32 -> fp16, round to nearest even; non-finite -> +0 and `nonfinite`; beyond the range -> +-65504 (E10)
ORBIT_RASTER_FN uint16_t env_half(float x, bool &nonfinite) {
    const uint32_t b = (uint32_t)float_bits(x), s = (b >> 16) & 0x8000u, a = b & 0x7FFFFFFFu;
    if (a >= 0x7F800000u) {
        nonfinite = true;
        return 0u;
    }
    if (a >= 0x477FF000u) return (uint16_t)(s | 0x7BFFu); // 65520 and above
    if (a < 0x33000000u) return (uint16_t)s;              // below 2^-25 (2^-25 itself ties to even: 0)
    uint32_t r, rem, half;
    if (a < 0x38800000u) { // below 2^-14: a multiple of 2^-24
        const uint32_t m = (a & 0x007FFFFFu) | 0x00800000u, shift = 126u - (a >> 23); // 14 .. 24
        r = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    } else {
        r = (a - 0x38000000u) >> 13, rem = a & 0x1FFFu, half = 0x1000u;
    }
    if (rem > half || (rem == half && (r & 1u))) r++;
    return (uint16_t)(s | r);
}
// fp16 -> fp32, exact
ORBIT_RASTER_FN float env_unhalf(uint16_t h) {
#ifdef __HIP_DEVICE_COMPILE__
    _Float16 v;
    __builtin_memcpy(&v, &h, 2);
    return (float)v;
#else
    const uint32_t s = ((uint32_t)h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    if (e == 0u) return bits_float((int32_t)s) + bits_float((int32_t)s | 0x33800000) * (float)m; // +-(m * 2^-24), exact
    if (e == 31u) return bits_float((int32_t)(s | 0x7F800000u | (m << 13)));
    return bits_float((int32_t)(s | ((e + 112u) << 23) | (m << 13)));
#endif
}
struct alignas(8) EnvTexel {
    uint16_t c[4];
};
// rgb (alpha 1) -> a texel; -> a channel was not finite
ORBIT_RASTER_FN bool env_store_rgb(const float *rgb, EnvTexel &t) {
    bool nonfinite = false;
    for (int k = 0; k < 3; k++) t.c[k] = env_half(rgb[k], nonfinite);
    t.c[3] = 0x3C00u;
    return nonfinite;
}

ORBIT_RASTER_FN uint32_t env_level_size(uint32_t size, uint32_t m) { return (size >> m) > 1u ? (size >> m) : 1u; }
ORBIT_RASTER_FN bool env_power_of_two(uint32_t v) { return v != 0u && (v & (v - 1u)) == 0u; }
ORBIT_RASTER_FN uint32_t env_full_levels(uint32_t size) { // floor(log2(size)) + 1
    uint32_t levels = 0u;
    for (uint32_t v = size; v != 0u; v >>= 1) levels++;
    return levels;
}

// A cube in E0's layout as the sampler sees it
struct EnvCube {
    const uint16_t *base;
    uint32_t size, levels;
    uint32_t offset[kEnvMaxLevels]; // texels in front of level m
};
// What the sampler tells whoever wants to count its cases: called with an index of orbit_host_c.h's census.  The kernels
// and every caller that hands nothing over get this one, which does nothing; the host mirror hands over its own.
struct EnvNoCensus {
    ORBIT_RASTER_FN void operator()(uint32_t) const {}
};
ORBIT_RASTER_FN EnvCube env_cube(const uint16_t *base, uint32_t size, uint32_t levels) {
    EnvCube c;
    c.base = base, c.size = size, c.levels = levels;
    uint32_t at = 0u;
    for (uint32_t m = 0; m < kEnvMaxLevels; m++) {
        c.offset[m] = m < levels ? at : 0u;
        const uint32_t n = env_level_size(size, m);
        if (m < levels) at += 6u * n * n; // at most 6 * 4096^2 * 4 / 3 < 2^28
    }
    return c;
}
ORBIT_RASTER_FN void env_layout(uint32_t sky_size, uint32_t irradiance_size, uint32_t prefiltered_size, uint32_t prefiltered_levels,
                                uint32_t brdf_size, OrbitEnvMapLayout &out) {
    out.sky_size = sky_size, out.sky_levels = env_full_levels(sky_size), out.irradiance_size = irradiance_size;
    out.prefiltered_size = prefiltered_size, out.prefiltered_levels = prefiltered_size ? prefiltered_levels : 0u, out.brdf_size = brdf_size;
    uint64_t sky = 0u, pre = 0u;
    for (uint32_t m = 0; m < kEnvMaxLevels; m++) {
        const bool s = m < out.sky_levels, p = m < out.prefiltered_levels;
        const uint32_t sn = env_level_size(sky_size, m), pn = env_level_size(prefiltered_size, m);
        out.sky_level_size[m] = s ? sn : 0u, out.sky_level_offset[m] = s ? (uint32_t)sky : 0u;
        out.prefiltered_level_size[m] = p ? pn : 0u, out.prefiltered_level_offset[m] = p ? (uint32_t)pre : 0u;
        if (s) sky += 6ull * sn * sn;
        if (p) pre += 6ull * pn * pn;
    }
    out.sky_texels = sky, out.irradiance_texels = 6ull * irradiance_size * irradiance_size, out.prefiltered_texels = pre;
    out.brdf_texels = (uint64_t)brdf_size * brdf_size;
}

// ---- the routines of E2, the project's own (Cephes' single-precision forms, every operation rounded on its own)
// atan of x >= 0 (+inf included)
ORBIT_RASTER_FN float env_atanc_pos(float x) {
    float y0, t;
    if (x > 2.414213562373095f)
        y0 = 1.5707963267948966f, t = -1.0f / x;
    else if (x > 0.4142135623730950f)
        y0 = 0.7853981633974483f, t = (x - 1.0f) / (x + 1.0f);
    else
        y0 = 0.0f, t = x;
    const float z = t * t;
    const float p = ((((8.05374449538e-2f * z - 1.38776856032e-1f) * z + 1.99777106478e-1f) * z - 3.33329491539e-1f) * z) * t + t;
    return y0 + p;
}
// GLSL atan(y, x): (0, 0) -> 0; the sign of a zero y is not looked at (y = -0, x < 0 -> +pi)
ORBIT_RASTER_FN float env_atan2c(float y, float x) {
    if (y == 0.0f && x == 0.0f) return 0.0f;
    float t = env_atanc_pos(fabsf(y) / fabsf(x));
    if (x < 0.0f) t = kShadePi - t;
    return y < 0.0f ? -t : t;
}
// asin of x in [-1, 1]; beyond: NaN
ORBIT_RASTER_FN float env_asinc(float x) {
    const float a = fabsf(x);
    if (!(a <= 1.0f)) return bits_float(0x7FC00000);
    const bool big = a > 0.5f;
    float z, t;
    if (big)
        z = 0.5f * (1.0f - a), t = sqrtf(z);
    else
        t = a, z = t * t;
    float r = (((((4.2163199048e-2f * z + 2.4181311049e-2f) * z + 4.5470025998e-2f) * z + 7.4953002686e-2f) * z + 1.6666752422e-1f) * z) * t + t;
    if (big) r = 1.5707963267948966f - (r + r);
    return x < 0.0f ? -r : r;
}

ORBIT_RASTER_FN void env_cross(const float *a, const float *b, float *out) { // GLSL cross
    out[0] = a[1] * b[2] - b[1] * a[2];
    out[1] = a[2] * b[0] - b[2] * a[0];
    out[2] = a[0] * b[1] - b[0] * a[1];
}

// ---- E1: in_local_pos of texel (px, py) of layer `face` of a level n texels wide.  The table: component k of the
// position is sign * (cx, cy, 1)[index], per layer
ORBIT_RASTER_FN void env_texel_direction(uint32_t face, uint32_t px, uint32_t py, uint32_t n, float *p) {
    const float cx = (2.0f * ((float)px + 0.5f)) / (float)n - 1.0f, cy = 1.0f - (2.0f * ((float)py + 0.5f)) / (float)n;
    switch (face) {
    case 0: p[0] = -1.0f, p[1] = cy, p[2] = cx; break;
    case 1: p[0] = 1.0f, p[1] = cy, p[2] = -cx; break;
    case 2: p[0] = -cx, p[1] = 1.0f, p[2] = cy; break;
    case 3: p[0] = -cx, p[1] = -1.0f, p[2] = -cy; break;
    case 4: p[0] = -cx, p[1] = cy, p[2] = -1.0f; break;
    default: p[0] = cx, p[1] = cy, p[2] = 1.0f; break;
    }
}

// ---- E2: one texel of the sky cube's level 0 from the panorama (w x h RGBA floats)
ORBIT_RASTER_FN uint32_t env_wrap(float fl, int step, uint32_t n) { // (floor + step) mod n; |floor| < 2^24
    const int r = ((int)fl + step) % (int)n;
    return (uint32_t)(r < 0 ? r + (int)n : r);
}
ORBIT_RASTER_FN void env_equirect_texel(const float *equirect, uint32_t w, uint32_t h, uint32_t face, uint32_t px, uint32_t py, uint32_t n,
                                        float *rgb) {
    float v[3];
    env_texel_direction(face, px, py, n, v);
    shade_normalize(v);
    const float u = env_atan2c(v[2], v[0]) * 0.1591f + 0.5f, t = 1.0f - (env_asinc(v[1]) * 0.3183f + 0.5f);
    const float sx = u * (float)w - 0.5f, sy = t * (float)h - 0.5f;
    const float flx = floorf(sx), fly = floorf(sy), fx = sx - flx, fy = sy - fly, gx = 1.0f - fx, gy = 1.0f - fy;
    const uint32_t x0 = env_wrap(flx, 0, w), x1 = env_wrap(flx, 1, w), y0 = env_wrap(fly, 0, h), y1 = env_wrap(fly, 1, h);
    const float *t00 = equirect + 4u * ((size_t)y0 * w + x0), *t10 = equirect + 4u * ((size_t)y0 * w + x1);
    const float *t01 = equirect + 4u * ((size_t)y1 * w + x0), *t11 = equirect + 4u * ((size_t)y1 * w + x1);
    for (int k = 0; k < 3; k++) rgb[k] = shade_clamp((t00[k] * gx + t10[k] * fx) * gy + (t01[k] * gx + t11[k] * fx) * fy, 0.0f, 10000.0f);
}

// ---- E3: texel (x, y) of a face of level m + 1 from the face of level m (n_src texels wide; n_src >= 2)
ORBIT_RASTER_FN bool env_mip_texel(const uint16_t *src_face, uint32_t n_src, uint32_t x, uint32_t y, EnvTexel &out) {
    const uint16_t *r0 = src_face + 4u * ((size_t)(2u * y) * n_src + 2u * x), *r1 = r0 + 4u * (size_t)n_src;
    bool nonfinite = false;
    for (int k = 0; k < 4; k++)
        out.c[k] = env_half(((env_unhalf(r0[k]) + env_unhalf(r0[4 + k])) + (env_unhalf(r1[k]) + env_unhalf(r1[4 + k]))) * 0.25f, nonfinite);
    return nonfinite;
}

// ---- E4: the cube sampler
// Vulkan's face selection: -> the layer; sc, tc, ma = |major axis|
ORBIT_RASTER_FN uint32_t env_face(const float *d, float &sc, float &tc, float &ma) {
    const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
    if (az >= ax && az >= ay) {
        const bool neg = d[2] < 0.0f;
        sc = neg ? -d[0] : d[0], tc = -d[1], ma = az;
        return neg ? 5u : 4u;
    }
    if (ay >= ax) {
        const bool neg = d[1] < 0.0f;
        sc = d[0], tc = neg ? -d[2] : d[2], ma = ay;
        return neg ? 3u : 2u;
    }
    const bool neg = d[0] < 0.0f;
    sc = neg ? d[2] : -d[2], tc = -d[1], ma = ax;
    return neg ? 1u : 0u;
}
// The texel a tap at (i, j) of `face` reads, i or j (not both) in -1 or n: across the edge, in integers.  A texel centre
// is the point (a, b, +-n) of the face's plane in units of 1 / n, a = 2 i + 1 - n; a tap one texel outside has |a| = n + 1
// and folds over the edge to the point with that axis at +-n and the old major axis at +-(n - 1).
ORBIT_RASTER_FN void env_fold(uint32_t &face, int &i, int &j, int n) {
    const int a = 2 * i + 1 - n, b = 2 * j + 1 - n;
    int P[3];
    switch (face) { // the inverse of the specification's table
    case 0: P[0] = n, P[1] = -b, P[2] = -a; break;
    case 1: P[0] = -n, P[1] = -b, P[2] = a; break;
    case 2: P[0] = a, P[1] = n, P[2] = b; break;
    case 3: P[0] = a, P[1] = -n, P[2] = -b; break;
    case 4: P[0] = a, P[1] = -b, P[2] = n; break;
    default: P[0] = -a, P[1] = -b, P[2] = -n; break;
    }
    // (constant indices only: the loops unroll into selects, nothing is indexed by a lane's value)
    const int major = (int)(face >> 1);
    int over = 0;
    for (int k = 0; k < 3; k++)
        if (k != major && (P[k] > n || P[k] < -n)) over = k;
    bool neg = false;
    for (int k = 0; k < 3; k++) {
        if (k == over) {
            neg = P[k] < 0;
            P[k] = neg ? -n : n;
        } else if (k == major) {
            P[k] = P[k] > 0 ? n - 1 : -(n - 1);
        }
    }
    face = 2u * (uint32_t)over + (neg ? 1u : 0u);
    int sc, tc;
    switch (face) {
    case 0: sc = -P[2], tc = -P[1]; break;
    case 1: sc = P[2], tc = -P[1]; break;
    case 2: sc = P[0], tc = P[2]; break;
    case 3: sc = P[0], tc = -P[2]; break;
    case 4: sc = P[0], tc = -P[1]; break;
    default: sc = -P[0], tc = -P[1]; break;
    }
    i = (sc + n - 1) >> 1, j = (tc + n - 1) >> 1;
}
ORBIT_RASTER_FN void env_load_rgb(const EnvCube &c, uint32_t level, uint32_t n, uint32_t face, int i, int j, float *rgb) {
    uint32_t offset = 0u; // a select per level, not a load indexed by the lane's level
    for (uint32_t m = 0; m < kEnvMaxLevels; m++)
        if (m == level) offset = c.offset[m];
    const uint16_t *p = c.base + 4u * ((size_t)offset + ((size_t)face * n + (size_t)j) * n + (size_t)i);
    EnvTexel t;
    __builtin_memcpy(&t, __builtin_assume_aligned(p, 8), 8);
    for (int k = 0; k < 3; k++) rgb[k] = env_unhalf(t.c[k]);
}
// the tap (i, j) of a face of level `level` (n wide), i and j in -1 .. n
template <class Census = EnvNoCensus>
ORBIT_RASTER_FN void env_tap(const EnvCube &c, uint32_t level, uint32_t n, uint32_t face, int i, int j, float *rgb, const Census &census = Census()) {
    const int in = (int)n;
    const bool out_x = i < 0 || i >= in, out_y = j < 0 || j >= in;
    if (!out_x && !out_y) {
        env_load_rgb(c, level, n, face, i, j, rgb);
        return;
    }
    const int ci = i < 0 ? 0 : i >= in ? in - 1 : i, cj = j < 0 ? 0 : j >= in ? in - 1 : j;
    if (out_x != out_y) {
        census(6u + 4u * face + (out_x ? (i < 0 ? 0u : 1u) : (j < 0 ? 2u : 3u)));
        env_fold(face, i, j, in);
        env_load_rgb(c, level, n, face, i, j, rgb);
        return;
    }
    // the corner: the three texels that meet there
    census(30u + 4u * face + (i < 0 ? 0u : 1u) + (j < 0 ? 0u : 2u));
    float own[3], ax[3], ay[3];
    env_load_rgb(c, level, n, face, ci, cj, own);
    uint32_t fx = face, fy = face;
    int xi = i, xj = cj, yi = ci, yj = j;
    env_fold(fx, xi, xj, in);
    env_fold(fy, yi, yj, in);
    env_load_rgb(c, level, n, fx, xi, xj, ax);
    env_load_rgb(c, level, n, fy, yi, yj, ay);
    for (int k = 0; k < 3; k++) rgb[k] = ((own[k] + ax[k]) + ay[k]) / 3.0f;
}
template <class Census = EnvNoCensus>
ORBIT_RASTER_FN void env_sample_level(const EnvCube &c, uint32_t level, uint32_t face, float s, float t, float *rgb, const Census &census = Census()) {
    const uint32_t n = env_level_size(c.size, level);
    const float x = s * (float)n - 0.5f, y = t * (float)n - 0.5f;
    const float flx = floorf(x), fly = floorf(y), fx = x - flx, fy = y - fly, gx = 1.0f - fx, gy = 1.0f - fy;
    const int i0 = (int)flx, j0 = (int)fly; // s, t in [0, 1]: -1 .. n - 1
    float t00[3], t10[3], t01[3], t11[3];
    env_tap(c, level, n, face, i0, j0, t00, census), env_tap(c, level, n, face, i0 + 1, j0, t10, census);
    env_tap(c, level, n, face, i0, j0 + 1, t01, census), env_tap(c, level, n, face, i0 + 1, j0 + 1, t11, census);
    for (int k = 0; k < 3; k++) rgb[k] = (t00[k] * gx + t10[k] * fx) * gy + (t01[k] * gx + t11[k] * fx) * fy;
}
// textureLod(cube, d, lod).rgb -> the direction was good
template <class Census = EnvNoCensus>
ORBIT_RASTER_FN bool env_sample(const EnvCube &c, const float *d, float lod, float *rgb, const Census &census = Census()) {
    const bool finite = fabsf(d[0]) < INFINITY && fabsf(d[1]) < INFINITY && fabsf(d[2]) < INFINITY; // false for NaN
    if (!finite || (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f)) {
        rgb[0] = rgb[1] = rgb[2] = 0.0f;
        return false;
    }
    float sc, tc, ma;
    const uint32_t face = env_face(d, sc, tc, ma);
    census(face);
    const float s = (0.5f * sc) / ma + 0.5f, t = (0.5f * tc) / ma + 0.5f;
    const float top = (float)(c.levels - 1u);
    if (!(lod > 0.0f)) lod = 0.0f;
    if (lod > top) lod = top;
    const float lf = floorf(lod), f = lod - lf;
    const uint32_t l = (uint32_t)lf;
    env_sample_level(c, l, face, s, t, rgb, census);
    if (f != 0.0f) { // then l < levels - 1
        census(60u);
        float next[3];
        env_sample_level(c, l + 1u, face, s, t, next, census);
        const float g = 1.0f - f;
        for (int k = 0; k < 3; k++) rgb[k] = rgb[k] * g + next[k] * f;
    }
    return true;
}

// ---- E5: one texel of the irradiance cube -> its colour; bad: E4's bad directions among its taps
ORBIT_RASTER_FN float env_irradiance_lod(uint32_t sky_size, uint32_t irradiance_size) {
    return shade_max(0.0f, shade_log2c((float)sky_size / (float)irradiance_size));
}
template <class Census = EnvNoCensus>
ORBIT_RASTER_FN void env_irradiance_texel(const EnvCube &sky, float lod, float sample_delta, uint32_t face, uint32_t px, uint32_t py, uint32_t n,
                                          float *rgb, uint64_t &bad, const Census &census = Census()) {
    float p[3], normal[3], right[3], up[3] = {0.0f, 1.0f, 0.0f};
    env_texel_direction(face, px, py, n, p);
    for (int k = 0; k < 3; k++) normal[k] = p[k];
    shade_normalize(normal);
    env_cross(up, normal, right);
    shade_normalize(right);
    env_cross(normal, right, up);
    shade_normalize(up);
    float sum[3] = {0.0f, 0.0f, 0.0f}, count = 0.0f;
    const float two_pi = 2.0f * kShadePi, half_pi = 0.5f * kShadePi;
    for (float phi = 0.0f; phi < two_pi; phi += sample_delta) {
        float sp, cp;
        shadow_sincos(phi, sp, cp);
        for (float theta = 0.0f; theta < half_pi; theta += sample_delta) {
            float st, ct, d[3], c[3];
            shadow_sincos(theta, st, ct);
            const float tx = st * cp, ty = st * sp;
            for (int k = 0; k < 3; k++) d[k] = (tx * right[k] + ty * up[k]) + ct * p[k];
            if (!env_sample(sky, d, lod, c, census)) bad++;
            for (int k = 0; k < 3; k++) sum[k] = sum[k] + (c[k] * ct) * st;
            count = count + 1.0f;
        }
    }
    const float scale = 1.0f / count;
    for (int k = 0; k < 3; k++) rgb[k] = (kShadePi * sum[k]) * scale;
}

// ---- E6: the prefiltered cube
ORBIT_RASTER_FN float env_radical_inverse(uint32_t i) { // hammersley_2d's second component
    uint32_t bits = (i << 16) | (i >> 16);
    bits = ((bits & 0x55555555u) << 1) | ((bits & 0xAAAAAAAAu) >> 1);
    bits = ((bits & 0x33333333u) << 2) | ((bits & 0xCCCCCCCCu) >> 2);
    bits = ((bits & 0x0F0F0F0Fu) << 4) | ((bits & 0xF0F0F0F0u) >> 4);
    bits = ((bits & 0x00FF00FFu) << 8) | ((bits & 0xFF00FF00u) >> 8);
    return (float)bits * 2.3283064365386963e-10f;
}
ORBIT_RASTER_FN float env_roughness(uint32_t level, uint32_t levels) { return levels > 1u ? (float)level / (float)(levels - 1u) : 0.0f; }
// what depends on the sample and the roughness alone: (2 pi) * Xi.x, cosTheta, sinTheta
ORBIT_RASTER_FN void env_ggx_entry(uint32_t i, uint32_t sample_count, float roughness, float &phi0, float &cos_theta, float &sin_theta) {
    const float xi_x = (float)i / (float)sample_count, xi_y = env_radical_inverse(i);
    const float alpha = roughness * roughness;
    phi0 = (2.0f * kShadePi) * xi_x;
    cos_theta = sqrtf((1.0f - xi_y) / (1.0f + (alpha * alpha - 1.0f) * xi_y));
    sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
}
ORBIT_RASTER_FN float env_random(float x, float y) { // functions.glsl random(vec2)
    const float dt = x * 12.9898f + y * 78.233f;
    const float sn = dt - 3.14f * floorf(dt / 3.14f);
    float s, c;
    shadow_sincos(sn, s, c);
    const float v = s * 43758.5453f;
    return v - floorf(v);
}
// the tangent frame of importance_sample_ggx around `normal` (both shaders'; normalise_y: functions.glsl's normalises tangentY)
ORBIT_RASTER_FN bool env_ggx_frame(const float *normal, bool normalise_y, float *tangent_x, float *tangent_y) {
    const bool z_up = fabsf(normal[2]) < 0.999f; // E12
    const float up[3] = {z_up ? 0.0f : 1.0f, 0.0f, z_up ? 1.0f : 0.0f};
    env_cross(up, normal, tangent_x);
    shade_normalize(tangent_x);
    env_cross(normal, tangent_x, tangent_y);
    if (normalise_y) shade_normalize(tangent_y);
    return z_up;
}
// what depends on the texel alone: N, the frame and random's phase
struct EnvPrefilterTexel {
    float N[3], tangent_x[3], tangent_y[3], phase, sum[3], weight;
    bool z_up;
};
ORBIT_RASTER_FN void env_prefilter_begin(uint32_t face, uint32_t px, uint32_t py, uint32_t n, EnvPrefilterTexel &t) {
    env_texel_direction(face, px, py, n, t.N);
    shade_normalize(t.N);
    t.z_up = env_ggx_frame(t.N, true, t.tangent_x, t.tangent_y);
    t.phase = env_random(t.N[0], t.N[2]) * 0.1f;
    t.sum[0] = t.sum[1] = t.sum[2] = 0.0f, t.weight = 0.0f;
}
struct EnvPrefilterLevel { // one per launch
    float roughness, a2, a2_minus_1, samples_f, omega_p;
};
ORBIT_RASTER_FN EnvPrefilterLevel env_prefilter_level(uint32_t level, uint32_t levels, uint32_t sample_count, uint32_t sky_size) {
    EnvPrefilterLevel l;
    l.roughness = env_roughness(level, levels);
    const float a = l.roughness * l.roughness, dim = (float)sky_size;
    l.a2 = a * a, l.a2_minus_1 = l.a2 - 1.0f, l.samples_f = (float)sample_count;
    l.omega_p = (4.0f * kShadePi) / ((6.0f * dim) * dim);
    return l;
}
// one sample of one texel -> 0: dotNL <= 0, 1: it was added, 2: it was added and its direction was bad
template <class Census = EnvNoCensus>
ORBIT_RASTER_FN uint32_t env_prefilter_sample(const EnvCube &sky, const EnvPrefilterLevel &l, float phi0, float cos_theta, float sin_theta,
                                              EnvPrefilterTexel &t, const Census &census = Census()) {
    float s, c, H[3], L[3], rgb[3];
    shadow_sincos(phi0 + t.phase, s, c);
    const float hx = sin_theta * c, hy = sin_theta * s;
    for (int k = 0; k < 3; k++) H[k] = (t.tangent_x[k] * hx + t.tangent_y[k] * hy) + t.N[k] * cos_theta;
    shade_normalize(H);
    const float vh = shade_dot(t.N, H), vh2 = 2.0f * vh; // V = N
    for (int k = 0; k < 3; k++) L[k] = vh2 * H[k] - t.N[k];
    const float ndl = shade_clamp(shade_dot(t.N, L), 0.0f, 1.0f);
    if (!(ndl > 0.0f)) return 0u;
    const float ndh = shade_clamp(vh, 0.0f, 1.0f); // dotNH and dotVH: the same expression
    float den = (ndh * ndh) * l.a2_minus_1 + 1.0f;
    den = (kShadePi * den) * den;
    const float D = l.a2 / shade_max(den, kShadeEps);
    const float pdf = (D * ndh) / (4.0f * ndh) + 0.0001f;
    const float omega_s = 1.0f / (l.samples_f * pdf);
    const float mip = l.roughness == 0.0f ? 0.0f : shade_max(0.5f * shade_log2c(omega_s / l.omega_p) + 1.0f, 0.0f);
    const bool good = env_sample(sky, L, mip, rgb, census);
    for (int k = 0; k < 3; k++) t.sum[k] = t.sum[k] + rgb[k] * ndl;
    t.weight = t.weight + ndl;
    return good ? 1u : 2u;
}
ORBIT_RASTER_FN void env_prefilter_end(const EnvPrefilterTexel &t, float *rgb) {
    for (int k = 0; k < 3; k++) rgb[k] = t.sum[k] / t.weight;
}

// ---- E7: one texel of the BRDF table -> A, B
ORBIT_RASTER_FN float env_schlick_ggx(float ndv, float roughness) { // brdf_integration.frag's own
    const float k = (roughness * roughness) / 2.0f;
    return ndv / (ndv * (1.0f - k) + k);
}
ORBIT_RASTER_FN void env_brdf_texel(uint32_t x, uint32_t y, uint32_t n, uint32_t sample_count, float *ab) {
    const float ndv = ((float)x + 0.5f) / (float)n, roughness = ((float)y + 0.5f) / (float)n;
    const float V[3] = {sqrtf(1.0f - ndv * ndv), 0.0f, ndv}, N[3] = {0.0f, 0.0f, 1.0f};
    float tangent[3], bitangent[3], A = 0.0f, B = 0.0f;
    env_ggx_frame(N, false, tangent, bitangent);
    const float g_v = env_schlick_ggx(shade_max(shade_dot(N, V), 0.0f), roughness);
    for (uint32_t i = 0; i < sample_count; i++) {
        float phi, cos_theta, sin_theta, s, c, H[3], L[3];
        env_ggx_entry(i, sample_count, roughness, phi, cos_theta, sin_theta);
        shadow_sincos(phi, s, c);
        const float hx = c * sin_theta, hy = s * sin_theta;
        for (int k = 0; k < 3; k++) H[k] = (tangent[k] * hx + bitangent[k] * hy) + N[k] * cos_theta;
        shade_normalize(H);
        const float vh = shade_dot(V, H), vh2 = 2.0f * vh;
        for (int k = 0; k < 3; k++) L[k] = vh2 * H[k] - V[k];
        shade_normalize(L);
        const float ndl = shade_max(L[2], 0.0f), ndh = shade_max(H[2], 0.0f), vdh = shade_max(vh, 0.0f);
        if (ndl > 0.0f) {
            const float G = env_schlick_ggx(shade_max(shade_dot(N, L), 0.0f), roughness) * g_v;
            const float g_vis = (G * vdh) / (ndh * ndv);
            const float fc = post_powc(1.0f - vdh, 5.0f);
            A = A + (1.0f - fc) * g_vis;
            B = B + fc * g_vis;
        }
    }
    ab[0] = A / (float)sample_count, ab[1] = B / (float)sample_count;
}

// ---- E9, for the entry points and the mirror: nullptr, or what is wrong
// The smallest sample_delta: 1 257 x 315 trips per irradiance texel, 25 times the reference's 252 x 63 at 0.025.  A thread
// runs its texel's trips one after the other, so the bound is what keeps one launch's length in hand, not only finite.
constexpr float kEnvMinSampleDelta = 0.005f;
// [a, a + a_bytes) and [b, b + b_bytes) share a byte; a NULL or empty range shares none
inline bool env_ranges_overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    if (!a || !b || a_bytes == 0u || b_bytes == 0u) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + b_bytes && pb < pa + a_bytes;
}
inline const char *env_map_check(const OrbitEnvMap &j) {
    if (j.flags != 0u || j._pad != 0u) return "unknown flags";
    if (!j.sky && !j.irradiance && !j.prefiltered && !j.brdf) return "no product asked for: sky, irradiance, prefiltered and brdf are all NULL";
    if (j.equirect && !j.sky) return "equirect without a sky cube to write";
    if ((j.irradiance || j.prefiltered) && !j.sky) return "irradiance or prefiltered without a sky cube";
    if (j.sky) {
        if (!env_power_of_two(j.sky_size) || j.sky_size > ORBIT_ENV_MAX_SIZE) return "sky_size is not a power of two in 1..4096";
        if (j.equirect && (j.equirect_w == 0u || j.equirect_h == 0u || j.equirect_w > 65536u || j.equirect_h > 65536u)) return "equirect size (1..65536 each)";
    }
    if (j.irradiance) {
        if (j.irradiance_size == 0u || j.irradiance_size > ORBIT_ENV_MAX_SIZE) return "irradiance_size (1..4096)";
        if (!(j.sample_delta >= kEnvMinSampleDelta && j.sample_delta < INFINITY)) return "sample_delta (finite, at least 0.005)";
    }
    if (j.prefiltered) {
        if (j.prefiltered_size == 0u || j.prefiltered_size > ORBIT_ENV_MAX_SIZE) return "prefiltered_size (1..4096)";
        if (j.prefiltered_levels == 0u || j.prefiltered_levels > ORBIT_ENV_MAX_LEVELS) return "prefiltered_levels (1..13)";
        if (j.sample_count == 0u || j.sample_count > ORBIT_ENV_MAX_SAMPLES) return "sample_count (1..65536)";
    }
    if (j.brdf) {
        if (j.brdf_size == 0u || j.brdf_size > ORBIT_ENV_MAX_SIZE) return "brdf_size (1..4096)";
        if (j.brdf_sample_count == 0u || j.brdf_sample_count > ORBIT_ENV_MAX_SAMPLES) return "brdf_sample_count (1..65536)";
    }
    if (((uintptr_t)j.equirect & 15u) || (((uintptr_t)j.sky | (uintptr_t)j.irradiance | (uintptr_t)j.prefiltered | (uintptr_t)j.stats) & 7u) ||
        ((uintptr_t)j.brdf & 3u))
        return "alignment: equirect 16 B, sky, irradiance, prefiltered and stats 8 B, brdf 4 B";
    OrbitEnvMapLayout lay; // the sizes of what is asked for have been checked above
    env_layout(j.sky ? j.sky_size : 0u, j.irradiance ? j.irradiance_size : 0u, j.prefiltered ? j.prefiltered_size : 0u, j.prefiltered_levels,
               j.brdf ? j.brdf_size : 0u, lay);
    const void *const buffers[6] = {j.equirect, j.sky, j.irradiance, j.prefiltered, j.brdf, j.stats};
    const uint64_t bytes[6] = {j.equirect ? 16ull * j.equirect_w * j.equirect_h : 0u, 8u * lay.sky_texels, 8u * lay.irradiance_texels,
                               8u * lay.prefiltered_texels, 4u * lay.brdf_texels, sizeof(OrbitEnvMapStats)};
    for (int a = 0; a < 6; a++)
        for (int b = a + 1; b < 6; b++)
            if (env_ranges_overlap(buffers[a], bytes[a], buffers[b], bytes[b])) return "two of the call's buffers share bytes";
    return nullptr;
}
inline const char *env_sample_check(const OrbitEnvSample &j) {
    if (j.flags != 0u) return "unknown flags";
    if (j.size == 0u || j.size > ORBIT_ENV_MAX_SIZE) return "size (1..4096)";
    if (j.levels == 0u || j.levels > ORBIT_ENV_MAX_LEVELS) return "levels (1..13)";
    if (!j.cube) return "cube is NULL";
    if (j.n != 0u && (!j.directions || !j.lods || !j.rgb)) return "directions, lods or rgb NULL";
    if ((((uintptr_t)j.cube | (uintptr_t)j.bad_directions) & 7u) || (((uintptr_t)j.directions | (uintptr_t)j.lods | (uintptr_t)j.rgb) & 3u))
        return "alignment: cube and bad_directions 8 B, directions, lods and rgb 4 B";
    const EnvCube cube = env_cube(j.cube, j.size, j.levels);
    uint64_t texels = 0u;
    for (uint32_t m = 0; m < j.levels; m++) texels = (uint64_t)cube.offset[m] + 6ull * env_level_size(j.size, m) * env_level_size(j.size, m);
    const void *const inputs[3] = {j.cube, j.directions, j.lods};
    const uint64_t input_bytes[3] = {8u * texels, 12ull * j.n, 4ull * j.n};
    for (int a = 0; a < 3; a++)
        if (env_ranges_overlap(j.rgb, 12ull * j.n, inputs[a], input_bytes[a]) || env_ranges_overlap(j.bad_directions, 8u, inputs[a], input_bytes[a]))
            return "an output shares bytes with an input";
    if (env_ranges_overlap(j.rgb, 12ull * j.n, j.bad_directions, 8u)) return "the two outputs share bytes";
    return nullptr;
}

} // namespace raster
} // namespace orbit
