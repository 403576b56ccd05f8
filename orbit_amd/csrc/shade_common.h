// shade_common.h — the arithmetic of orbit_fragments_shade (include/orbit_abi_ext.h L1-L9), written once
// for the device kernels (fragments_shade.hip) and the host mirror (orbit_amd/host/orbit_raster.cpp).  The pieces:
// shade_slice_canonical is L2's integer (log2c and f2u_sat restated for the host: orbit_device.h's are device only and
// this header does not depend on it); shade_cluster is L2's lookup; shade_light_row is what L5 / L6 read of a light;
// shade_pixel_begin / _light / _end are L3-L8 of one pixel; shade_walk_pixel is the whole of L1-L8 for a lane or a host
// loop that walks its own list, in the tier of any of the three shade calls (ShadeTier is this call's).  Equal inputs, equal functions: equal bytes.  What does not depend on the light is evaluated
// once per pixel: every operation is still rounded on its own, so where it is evaluated does not change a bit.
#pragma once
#include "../../include/orbit_abi_ext.h"
#include "surface_common.h" // finite_or_zero, and raster_common.h's float_bits / bits_float

namespace orbit {
namespace raster {

enum ShadeVerdict : uint32_t { kShadeWritten = 0, kShadeUnshaded = 1, kShadeStale = 2 }; // of a covered pixel
enum : uint32_t { kShadeOutside = 1u, kShadeDegenerate = 2u, kShadeTextured = 4u, kShadeUnserved = 8u }; // of a written one
constexpr float kShadeEps = 0.0001f, kShadePi = 3.14159265359f;
constexpr uint32_t kLightSky = 0u, kLightDirectional = 1u, kLightPoint = 2u, kNone = 0xFFFFFFFFu; // types.glsl:298-300

// GLSL max / min / clamp, as orbit_device.h's gmax family
ORBIT_RASTER_FN float shade_max(float x, float y) { return x < y ? y : x; }
ORBIT_RASTER_FN float shade_min(float x, float y) { return y < x ? y : x; }
ORBIT_RASTER_FN float shade_clamp(float x, float lo, float hi) { return shade_min(shade_max(x, lo), hi); }
ORBIT_RASTER_FN float shade_dot(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
ORBIT_RASTER_FN void shade_normalize(float *v) {
    const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    for (int i = 0; i < 3; i++) v[i] = v[i] / len;
}

// H6's and A4's sine and cosine, the project's own, of theta in [0, 2 pi]: quadrant reduction in two steps, then fixed polynomials
ORBIT_RASTER_FN void shadow_sincos(float theta, float &s, float &c) {
    const int k = (int)(theta * 0.636619772f + 0.5f);
    const float kf = (float)k;
    const float r = (theta - kf * 1.5703125f) - kf * 4.83826794897e-4f;
    const float w = r * r;
    const float sin_r = ((((-1.9515295891e-4f * w + 8.3321608736e-3f) * w) + -1.6666654611e-1f) * w) * r + r;
    const float cos_r = ((((2.443315711809948e-5f * w + -1.388731625493765e-3f) * w) + 4.166664568298827e-2f) * w) * w + (1.0f - 0.5f * w);
    switch (k & 3) {
    case 0: s = sin_r, c = cos_r; break;
    case 1: s = cos_r, c = -sin_r; break;
    case 2: s = -sin_r, c = -cos_r; break;
    default: s = -cos_r, c = sin_r; break;
    }
}

// R2's clip = M x (x, y, z, w), M column-major
ORBIT_RASTER_FN void shadow_project(const float *M, float x, float y, float z, float w, float *c) {
    for (int r = 0; r < 4; r++) c[r] = ((M[r] * x + M[4 + r] * y) + M[8 + r] * z) + M[12 + r] * w;
}

// uint(float): saturating, NaN -> 0 (orbit_device.h f2u_sat)
ORBIT_RASTER_FN uint32_t shade_f2u_sat(float f) {
    if (!(f > 0.0f)) return 0u;
    if (f >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)f;
}

// The canonical software log2 (orbit_device.h log2c, oracle/orbit_oracle.c orbit_log2f): exponent + degree-9 Horner
// polynomial, products and sums only
ORBIT_RASTER_FN float shade_log2c(float x) {
    uint32_t b = (uint32_t)float_bits(x);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return x;
    if ((b & 0x7FFFFFFFu) == 0u) return -INFINITY;
    if (b & 0x80000000u) return bits_float(0x7FC00000);
    if (b == 0x7F800000u) return x;
    int e = 0;
    if (b < 0x00800000u) {
        x = x * 16777216.0f;
        b = (uint32_t)float_bits(x);
        e = -24;
    }
    e += (int)(b >> 23) - 127;
    float m = bits_float((int32_t)((b & 0x007FFFFFu) | 0x3F800000u));
    if (m > 1.41421354f) {
        m = m * 0.5f;
        e += 1;
    }
    const float f = m - 1.0f;
    const float c[10] = {-0x1.cebep-4f,   0x1.80ab18p-3f,  -0x1.865ffcp-3f, 0x1.a265fcp-3f, -0x1.eac694p-3f,
                         0x1.2782e6p-2f,  -0x1.715a68p-2f, 0x1.ec708p-2f,   -0x1.71547p-1f, 0x1.715476p+0f};
    float p = c[0];
    for (int i = 1; i < 10; i++) {
        p = p * f;
        p = p + c[i];
    }
    const float r = p * f;
    return r + (float)e;
}

// L2's slice of a depth d: orbit_device.h's depth_slice_canonical of z_near / d
ORBIT_RASTER_FN uint32_t shade_slice_canonical(float z_near, float d, float z_scale, float z_bias) {
    return shade_f2u_sat(__builtin_fmaf(shade_log2c(z_near / d), z_scale, z_bias));
}

// L2's lookup of pixel (x, y) in slice `slice`: the walk [offset, offset + n) of the index list
struct ShadeCluster {
    uint32_t offset, n;
    bool outside, stale;
};
ORBIT_RASTER_FN ShadeCluster shade_cluster(const OrbitFragmentsShade &j, uint32_t x, uint32_t y, uint32_t slice) {
    ShadeCluster c = {0u, 0u, false, false};
    const uint32_t tx = x / j.tile_size_px, ty = y / j.tile_size_px;
    const uint32_t cx = j.cluster_count[0], cy = j.cluster_count[1], cz = j.cluster_count[2];
    if (tx >= cx || ty >= cy || slice >= cz) {
        c.outside = true;
        return c;
    }
    const uint32_t *pair = j.cluster_offset_image + 2u * ((size_t)tx + (size_t)ty * cx + (size_t)slice * cx * cy);
    c.offset = pair[0];
    c.n = pair[1] < ORBIT_SHADE_MAX_WALK ? pair[1] : ORBIT_SHADE_MAX_WALK;
    c.stale = (uint64_t)c.offset + c.n > (uint64_t)j.index_capacity;
    return c;
}
ORBIT_RASTER_FN const uint32_t *shade_indices(const OrbitFragmentsShade &j) {
    return (const uint32_t *)((const uint8_t *)j.light_index_buffer + ORBIT_LIGHT_INDEX_HEADER);
}

// What L5 / L6 read of a light, the colour already times the intensity: 16 words, a row of the staged form's table
struct alignas(16) ShadeLight {
    uint32_t type, shadow;
    float lc[3], intensity, position[3], inner_radius, direction[3], outer_radius;
    uint32_t _pad[2];
};
ORBIT_RASTER_FN void shade_light_row(const OrbitLightData &l, ShadeLight &out) {
    out.type = l.light_type, out.shadow = l.shadow_data_index;
    for (int i = 0; i < 3; i++) out.lc[i] = l.color[i] * l.intensity, out.position[i] = l.position[i], out.direction[i] = l.direction[i];
    out.intensity = l.intensity, out.inner_radius = l.inner_radius, out.outer_radius = l.outer_radius;
    out._pad[0] = out._pad[1] = 0u;
}

// A pixel under the walk: L3's factors, L4's V and what L6 needs of them for every light
struct ShadePixel {
    float wp[3], N[3], V[3], albedo[3], f0[3], one_minus_f0[3], sum[3];
    float one_minus_metallic, a2, a2_minus_1, k, one_minus_k, ndv, g_v, ndv4;
    bool textured, unserved;
};

ORBIT_RASTER_FN void shade_pixel_begin(const OrbitFragmentsShade &j, const OrbitMaterialData &m, const float *wp, const float *n, ShadePixel &px) {
    px.textured = m.base_texture_index != kNone || m.normal_texture_index != kNone || m.metallic_roughness_texture_index != kNone ||
                  m.occlusion_texture_index != kNone || m.emissive_texture_index != kNone; // L3
    px.unserved = false;
    const float metallic = m.metallic_factor, r = m.roughness_factor;
    for (int i = 0; i < 3; i++) {
        px.wp[i] = wp[i], px.N[i] = n[i], px.albedo[i] = m.base_color[i], px.sum[i] = m.emissive_factor[i];
        px.V[i] = j.view_pos[i] - wp[i]; // L4
    }
    shade_normalize(px.V);
    px.one_minus_metallic = 1.0f - metallic;
    for (int i = 0; i < 3; i++) {
        px.f0[i] = 0.04f * px.one_minus_metallic + px.albedo[i] * metallic;
        px.one_minus_f0[i] = 1.0f - px.f0[i];
    }
    const float a = r * r, rr = r + 1.0f;
    px.a2 = a * a, px.a2_minus_1 = px.a2 - 1.0f;
    px.k = (rr * rr) / 8.0f, px.one_minus_k = 1.0f - px.k;
    px.ndv = shade_max(shade_dot(px.N, px.V), kShadeEps);
    px.g_v = px.ndv / (px.ndv * px.one_minus_k + px.k);
    px.ndv4 = 4.0f * px.ndv;
}

// L5 and L6 of one light of the walk -> the light has a term, the L6_c it adds.  SHADOWS_SERVED (shadow_common.h): a
// shadowed directional light does not mark the pixel unserved
template <bool SHADOWS_SERVED = false>
ORBIT_RASTER_FN bool shade_light_term(const ShadeLight &l, float luminance_cutoff, ShadePixel &px, float *term) {
    float Ld[3], att;
    if (l.type == kLightPoint) {
        for (int i = 0; i < 3; i++) Ld[i] = l.position[i] - px.wp[i];
        float dist = sqrtf(shade_dot(Ld, Ld));
        for (int i = 0; i < 3; i++) Ld[i] = Ld[i] / dist;
        dist = shade_max(dist, l.inner_radius);
        const float d2 = dist * dist;
        att = shade_max(l.intensity / d2 - (luminance_cutoff * d2) / (l.outer_radius * l.outer_radius), 0.0f);
    } else if (l.type == kLightDirectional) {
        for (int i = 0; i < 3; i++) Ld[i] = l.direction[i];
        att = 1.0f;
        if (!SHADOWS_SERVED && l.shadow != kNone) px.unserved = true;
    } else {
        if (l.type == kLightSky) px.unserved = true;
        return false;
    }
    float H[3];
    for (int i = 0; i < 3; i++) H[i] = px.V[i] + Ld[i];
    shade_normalize(H);
    const float ndl = shade_max(shade_dot(px.N, Ld), kShadeEps), ndh = shade_max(shade_dot(px.N, H), 0.0f);
    const float hv = shade_max(shade_dot(H, px.V), 0.0f);
    float den = (ndh * ndh) * px.a2_minus_1 + 1.0f;
    den = (kShadePi * den) * den;
    const float D = px.a2 / shade_max(den, kShadeEps);
    const float G = px.g_v * (ndl / (ndl * px.one_minus_k + px.k));
    const float x = 1.0f - hv, p5 = ((x * x) * (x * x)) * x;
    const float DG = D * G, spec_den = px.ndv4 * ndl;
    for (int i = 0; i < 3; i++) {
        const float F = px.f0[i] + px.one_minus_f0[i] * p5;
        const float spec = (DG * F) / spec_den;
        const float kD = (1.0f - F) * px.one_minus_metallic;
        term[i] = ((((kD * px.albedo[i]) / kShadePi) + spec) * (l.lc[i] * att)) * ndl;
    }
    return true;
}
ORBIT_RASTER_FN void shade_pixel_light(const ShadeLight &l, float luminance_cutoff, ShadePixel &px) {
    float term[3];
    if (!shade_light_term(l, luminance_cutoff, px, term)) return;
    for (int i = 0; i < 3; i++) px.sum[i] = px.sum[i] + term[i];
}

// L7 and L8 of mode 0 -> the pixel was degenerate
ORBIT_RASTER_FN bool shade_pixel_end(const ShadePixel &px, float *color) {
    bool all_finite = true;
    for (int i = 0; i < 3; i++) {
        color[i] = px.sum[i];
        all_finite = finite_or_zero(color[i]) && all_finite;
    }
    color[3] = 1.0f;
    return !all_finite;
}

// L7 of mode 8: heat_colormap (functions.glsl:142-171) of n lights
ORBIT_RASTER_FN void shade_heat(uint32_t n, float *color) {
    const float x = shade_clamp((float)n / 32.0f, 0.0f, 1.0f);
    color[0] = shade_clamp(x < 0.7f ? 4.0f * x - 1.5f : -4.0f * x + 4.5f, 0.0f, 1.0f);
    color[1] = shade_clamp(x < 0.5f ? 4.0f * x - 0.5f : -4.0f * x + 3.5f, 0.0f, 1.0f);
    color[2] = shade_clamp(x < 0.3f ? 4.0f * x + 0.5f : -4.0f * x + 2.5f, 0.0f, 1.0f);
    color[3] = 1.0f;
}

// a table row into a value: on the device, where the entry point has checked the table's 16-B alignment, by 16-B loads
template <class Row>
ORBIT_RASTER_FN Row shade_load_row(const Row *table, uint32_t i) {
    Row r;
#ifdef __HIP_DEVICE_COMPILE__
    struct alignas(16) Quad {
        uint32_t w[4];
    };
    static_assert(sizeof(Row) % 16 == 0, "rows of whole quads");
    Quad q[sizeof(Row) / 16];
    const Quad *src = (const Quad *)(table + i);
    for (size_t k = 0; k < sizeof(Row) / 16; k++) q[k] = src[k];
    __builtin_memcpy(&r, q, sizeof(Row));
#else
    __builtin_memcpy(&r, table + i, sizeof(Row));
#endif
    return r;
}

// L1's verdict of a covered pixel's material word
ORBIT_RASTER_FN uint32_t shade_material_verdict(const OrbitFragmentsShade &j, uint32_t material) {
    return material == kNone ? kShadeUnshaded : material >= j.material_count ? kShadeStale : kShadeWritten;
}

// A tier is what one of the shade calls adds to the walk below: a policy type that holds no data on the device.  It names
// its Job and how to reach the base job in it, the Extra state a pixel carries beside ShadePixel, and reset (Extra of a
// pixel not yet begun: what an unwritten pixel counts and stores), begin (after shade_pixel_begin), light_checked (a
// light's row may be evaluated), light (L5 / L6 of one checked light), stale (the light just added made the pixel
// stale) and end (after shade_pixel_end).  This one is orbit_fragments_shade's: L1-L9 and nothing else.
struct ShadeTier {
    using Job = OrbitFragmentsShade;
    struct Extra {};
    ORBIT_RASTER_FN static const OrbitFragmentsShade &base(const Job &j) { return j; }
    ORBIT_RASTER_FN static void reset(Extra &) {}
    ORBIT_RASTER_FN void begin(const Job &, const OrbitMaterialData &, const float *, size_t, Extra &) const {}
    ORBIT_RASTER_FN static bool light_checked(const Job &, uint32_t, uint32_t) { return true; }
    ORBIT_RASTER_FN void light(const Job &j, const ShadeLight &l, uint32_t, uint32_t, ShadePixel &px, Extra &) const {
        shade_pixel_light(l, j.luminance_cutoff, px);
    }
    ORBIT_RASTER_FN static bool stale(const Extra &) { return false; }
    ORBIT_RASTER_FN static void end(Extra &) {}
};

// L7 and L8 of a pixel whose walk of n lights is over -> its marks
template <class Tier>
ORBIT_RASTER_FN uint32_t shade_walk_end(const OrbitFragmentsShade &b, bool outside, uint32_t n, const ShadePixel &px, float *color,
                                        typename Tier::Extra &e) {
    uint32_t marks = (outside ? kShadeOutside : 0u) | (px.textured ? kShadeTextured : 0u);
    if (b.render_mode == 0u) {
        if (shade_pixel_end(px, color)) marks |= kShadeDegenerate;
        if (px.unserved) marks |= kShadeUnserved;
        Tier::end(e);
    } else {
        shade_heat(n, color);
    }
    return marks;
}

// L1-L8 of covered pixel p = (x, y) whose slice is `slice`, walking its own list, in tier t (e reset by the caller) -> the
// verdict; kShadeWritten: color, n = lights_walked, marks = kShadeOutside | kShadeDegenerate | kShadeTextured |
// kShadeUnserved, and what the tier keeps in e
template <class Tier>
ORBIT_RASTER_FN uint32_t shade_walk_pixel(const Tier &t, const typename Tier::Job &j, uint32_t x, uint32_t y, size_t p, uint32_t slice,
                                          float *color, uint32_t &n, uint32_t &marks, typename Tier::Extra &e) {
    const OrbitFragmentsShade &b = Tier::base(j);
    n = 0u, marks = 0u;
    for (int i = 0; i < 4; i++) color[i] = 0.0f;
    const uint32_t material = b.material[p];
    const uint32_t verdict = shade_material_verdict(b, material);
    if (verdict != kShadeWritten) return verdict;
    const ShadeCluster c = shade_cluster(b, x, y, slice);
    if (c.stale) return kShadeStale;
    const uint32_t *walk = shade_indices(b) + c.offset;
    const OrbitMaterialData m = shade_load_row(b.materials, material);
    ShadePixel px;
    float wp[4], nrm[3];
    __builtin_memcpy(wp, b.world_pos + 4u * p, 16);
    __builtin_memcpy(nrm, b.normal + 3u * p, 12);
    shade_pixel_begin(b, m, wp, nrm, px);
    t.begin(j, m, wp, p, e);
    for (uint32_t i = 0; i < c.n; i++) {
        const uint32_t index = walk[i];
        if (index >= b.light_count) return kShadeStale;
        if (b.render_mode != 0u) { // the type and the shadow index for the tier's check, nothing else of the row
            if (!Tier::light_checked(j, b.lights[index].light_type, b.lights[index].shadow_data_index)) return kShadeStale;
            continue;
        }
        ShadeLight l;
        shade_light_row(shade_load_row(b.lights, index), l);
        if (!Tier::light_checked(j, l.type, l.shadow)) return kShadeStale;
        t.light(j, l, x, y, px, e);
        if (Tier::stale(e)) return kShadeStale;
    }
    n = c.n;
    marks = shade_walk_end<Tier>(b, c.outside, n, px, color, e);
    return kShadeWritten;
}

} // namespace raster
} // namespace orbit
