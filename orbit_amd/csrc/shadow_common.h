// shadow_common.h — the shadow arithmetic of orbit_fragments_shade_shadowed (include/orbit_abi_ext.h H1-H10, DESIGN.md
// §4.26), written once for the device kernels (fragments_shade_shadowed.hip) and the host mirror
// (orbit_amd/host/orbit_raster.cpp), on top of shade_common.h's L1-L9.  The pieces: shadow_theta is H6's noise (its sine
// and cosine, shadow_sincos, and R2's shadow_project live in shade_common.h, where ssao_common.h finds them too);
// shadow_eval is H2-H8 of one shadowed light at one pixel; shadow_light_checked is H1's range check; shadow_pixel_light is
// L5 / L6 / H9 of one light of the walk; ShadowedTier hands them to shade_common.h's walk.  Equal inputs, equal functions: equal bytes.
#pragma once
#include "shade_common.h"

namespace orbit {
namespace raster {

constexpr uint32_t kShadowNoCascade = 4u, kShadowBlockerTaps = 12u, kShadowFilterTaps = 32u;
enum : uint32_t { kShadowEvaluated = 1u, kShadowOutOfCascades = 2u, kShadowEarlyOut = 4u }; // of a written pixel

// poisson_offsets[0..31] of forward.frag:14-79 as (x, y) pairs; entries 32-63 are never read
constexpr float kShadowPoisson[2 * kShadowFilterTaps] = {
    0.0617981f,   0.07294159f, 0.6470215f,   0.7474022f,  -0.5987766f, -0.7512833f, -0.693034f,  0.6913887f,
    0.6987045f,   -0.6843052f, -0.9402866f,  0.04474335f, 0.8934509f,  0.07369385f, 0.1592735f,  -0.9686295f,
    -0.05664673f, 0.995282f,   -0.1203411f,  -0.1301079f, 0.1741608f,  -0.1682285f, -0.09369049f, 0.3196758f,
    0.185363f,    0.3213367f,  -0.1493771f,  -0.3147511f, 0.4452095f,  0.2580113f,  -0.1080467f, -0.5329178f,
    0.1604507f,   0.5460774f,  -0.4037193f,  -0.2611179f, 0.5947998f,  -0.2146744f, 0.3276062f,  0.9244621f,
    -0.6518704f,  -0.2503952f, -0.3580975f,  0.2806469f,  0.8587891f,  0.4838005f,  -0.1596546f, -0.8791054f,
    -0.3096867f,  0.5588146f,  -0.5128918f,  0.1448544f,  0.8581337f,  -0.424046f,  0.1562584f,  -0.5610626f,
    -0.7647934f,  0.2709858f,  -0.3090832f,  0.9020988f,  0.3935608f,  0.4609676f,  0.3929337f,  -0.5010948f};

// H6: theta of the pixel (x, y)
ORBIT_RASTER_FN float shadow_fract(float a) { return a - floorf(a); }
ORBIT_RASTER_FN float shadow_theta(uint32_t x, uint32_t y) {
    const float sx = (float)x + 0.5f, sy = (float)y + 0.5f;
    const float ign = shadow_fract(52.9829189f * shadow_fract(sx * 0.06711056f + sy * 0.00583715f));
    return (ign * 2.0f) * kShadePi;
}

// clamp((int)f, 0, res - 1) of an f that is floorf's, the conversion saturating, NaN -> 0
ORBIT_RASTER_FN uint32_t shadow_texel(float f, uint32_t res) {
    if (!(f > 0.0f)) return 0u;
    if (f >= (float)res) return res - 1u;
    return (uint32_t)f;
}

struct ShadowResult {
    float shadow;
    uint32_t cascade; // 0..3, kShadowNoCascade
    bool stale, early_out;
};

// H2-H8 of a shadowed light (its row in range by H1) at pixel (x, y): wp its four world_pos floats, N its normal
ORBIT_RASTER_FN ShadowResult shadow_eval(const OrbitFragmentsShadeShadowed &j, const OrbitShadowData *row, const float *wp, const float *N,
                                         const float *direction, float inner_radius, uint32_t x, uint32_t y) {
    ShadowResult out = {1.0f, kShadowNoCascade, false, false};
    for (uint32_t i = 0; i < 4u; i++) { // H2
        float c[4], q[4];
        shadow_project(row->light_projection_matrices[i], wp[0], wp[1], wp[2], wp[3], c);
        for (int k = 0; k < 4; k++) q[k] = c[k] / c[3];
        const bool inside = q[0] >= -1.0f && q[1] >= -1.0f && q[2] >= 0.0f && q[3] >= 0.0f && q[0] <= 1.0f && q[1] <= 1.0f && q[2] <= 1.0f && q[3] <= 1.0f;
        if (inside) {
            out.cascade = i;
            break;
        }
    }
    if (out.cascade == kShadowNoCascade) return out;
    const uint32_t map = row->shadow_map_indices[out.cascade]; // H3
    if (map >= j.shadow_map_count) {
        out.stale = true;
        return out;
    }
    const uint32_t res = j.shadow_resolution;
    const float resf = (float)res, texel = 1.0f / resf;
    const float *texels = j.shadow_maps + (size_t)map * res * res;
    const float ndl = shade_dot(N, direction); // H4
    const float nos = shade_clamp(1.0f - ndl, 0.0f, 1.0f);
    const float scale = (texel * j.normal_bias_scale) * nos, ob = ndl > 0.0f ? -j.oriented_bias : j.oriented_bias;
    float sp[3], c[4];
    for (int k = 0; k < 3; k++) sp[k] = (wp[k] + scale * N[k]) + ob * direction[k];
    shadow_project(row->light_projection_matrices[out.cascade], sp[0], sp[1], sp[2], 1.0f, c); // H5
    const float z = c[2] / c[3];
    const float u = (c[0] / c[3] + 1.0f) * 0.5f, v = ((c[1] / c[3]) * -1.0f + 1.0f) * 0.5f;
    const float inv_ws = 1.0f / row->shadow_map_world_sizes[out.cascade];
    const float light_uv = inner_radius * inv_ws;
    float s, cs; // H6
    shadow_sincos(shadow_theta(x, y), s, cs);
    const float rad = j.blocker_search_radius * inv_ws; // H7
    float avg = 0.0f;
    uint32_t count = 0u;
    for (uint32_t i = 0; i < kShadowBlockerTaps; i++) {
        const float ox = kShadowPoisson[2u * i], oy = kShadowPoisson[2u * i + 1u];
        const float rx = cs * ox + (-s) * oy, ry = s * ox + cs * oy;
        const float su = u + (rx * rad) * inv_ws, sv = v + (ry * rad) * inv_ws;
        const float t = texels[(size_t)shadow_texel(floorf(sv * resf), res) * res + shadow_texel(floorf(su * resf), res)];
        if (t > z) {
            avg = avg + (1.0f - t);
            count++;
        }
    }
    if (count == 0u || count == kShadowBlockerTaps) {
        out.shadow = count == 0u ? 1.0f : 0.0f;
        out.early_out = true;
        return out;
    }
    avg = avg / (float)count;
    const float pen = (((1.0f - z) - avg) / avg) * light_uv; // H8
    const float fr = shade_max(pen * inv_ws, texel);
    uint32_t lit = 0u;
    for (uint32_t i = 0; i < kShadowFilterTaps; i++) {
        const float ox = kShadowPoisson[2u * i], oy = kShadowPoisson[2u * i + 1u];
        const float rx = cs * ox + (-s) * oy, ry = s * ox + cs * oy;
        const float fx = floorf((u + rx * fr) * resf - 0.5f), fy = floorf((v + ry * fr) * resf - 0.5f);
        const uint32_t x0 = shadow_texel(fx, res), x1 = shadow_texel(fx + 1.0f, res);
        const size_t y0 = (size_t)shadow_texel(fy, res) * res, y1 = (size_t)shadow_texel(fy + 1.0f, res) * res;
        lit += (z >= texels[y0 + x0] ? 1u : 0u) + (z >= texels[y0 + x1] ? 1u : 0u) + (z >= texels[y1 + x0] ? 1u : 0u) +
               (z >= texels[y1 + x1] ? 1u : 0u);
    }
    out.shadow = (float)lit / 128.0f;
    return out;
}

// H1: a light of the walk (its type and shadow_data_index) names a shadow row in range, or none
ORBIT_RASTER_FN bool shadow_light_checked(const OrbitFragmentsShadeShadowed &j, uint32_t type, uint32_t shadow) {
    return type != kLightDirectional || shadow == kNone || shadow - j.shadow_index_base < j.shadow_count;
}

// What H adds to a pixel under the walk: H10's planes and counters, and world_pos' fourth float
struct ShadowPixel {
    float w, factor;
    uint32_t cascade, evaluations, marks;
    bool stale;
};
ORBIT_RASTER_FN void shadow_pixel_begin(float w, ShadowPixel &sp) {
    sp.w = w, sp.factor = 1.0f, sp.cascade = kNone, sp.evaluations = 0u, sp.marks = 0u, sp.stale = false;
}

// L5, L6 and H9 of one light of the walk, shadow_light_checked
ORBIT_RASTER_FN void shadow_pixel_light(const OrbitFragmentsShadeShadowed &j, const ShadeLight &l, uint32_t x, uint32_t y, ShadePixel &px,
                                        ShadowPixel &sp) {
    float term[3];
    if (!shade_light_term<true>(l, j.shade.luminance_cutoff, px, term)) return;
    if (l.type == kLightDirectional) {
        float shadow = 1.0f;
        if (l.shadow != kNone) {
            const float wp[4] = {px.wp[0], px.wp[1], px.wp[2], sp.w};
            const ShadowResult e = shadow_eval(j, j.shadows + (l.shadow - j.shadow_index_base), wp, px.N, l.direction, l.inner_radius, x, y);
            if (e.stale) {
                sp.stale = true;
                return;
            }
            if (sp.evaluations == 0u) sp.factor = e.shadow, sp.cascade = e.cascade;
            sp.evaluations++;
            sp.marks |= kShadowEvaluated | (e.cascade == kShadowNoCascade ? kShadowOutOfCascades : 0u) | (e.early_out ? kShadowEarlyOut : 0u);
            shadow = e.shadow;
        }
        for (int i = 0; i < 3; i++) term[i] = term[i] * shadow;
    }
    for (int i = 0; i < 3; i++) px.sum[i] = px.sum[i] + term[i];
}

// orbit_fragments_shade_shadowed's tier of shade_common.h's walk
struct ShadowedTier {
    using Job = OrbitFragmentsShadeShadowed;
    using Extra = ShadowPixel;
    ORBIT_RASTER_FN static const OrbitFragmentsShade &base(const Job &j) { return j.shade; }
    ORBIT_RASTER_FN static void reset(Extra &sp) { shadow_pixel_begin(1.0f, sp); }
    ORBIT_RASTER_FN void begin(const Job &, const OrbitMaterialData &, const float *wp, size_t, Extra &sp) const { sp.w = wp[3]; }
    ORBIT_RASTER_FN static bool light_checked(const Job &j, uint32_t type, uint32_t shadow) { return shadow_light_checked(j, type, shadow); }
    ORBIT_RASTER_FN void light(const Job &j, const ShadeLight &l, uint32_t x, uint32_t y, ShadePixel &px, Extra &sp) const {
        shadow_pixel_light(j, l, x, y, px, sp);
    }
    ORBIT_RASTER_FN static bool stale(const Extra &sp) { return sp.stale; }
    ORBIT_RASTER_FN static void end(Extra &sp) { finite_or_zero(sp.factor); }
};

} // namespace raster
} // namespace orbit
