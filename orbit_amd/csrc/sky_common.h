// sky_common.h — the arithmetic of orbit_fragments_shade_sky (include/orbit_abi_ext.h K1-K10), written
// once for the device kernels (fragments_shade_sky.hip) and the host mirror (orbit_amd/host/orbit_raster.cpp), on top of
// shade_common.h's L1-L9, shadow_common.h's H1-H10 and env_common.h's E4, none of which it changes.  The pieces: sky_table is
// K6; sky_pixel_begin K8; sky_light_term K2-K7 of one SKY light at one pixel; sky_pixel_light K1 in front of
// shadow_pixel_light; SkyTier hands them to shade_common.h's walk; sky_box_pixel K9; sky_check the argument errors, for
// the entry point and the mirror alike.  fp32, every operation rounded on its own.  Equal inputs, equal functions: equal bytes.
#pragma once
#include "shade_common.h"
#include "shadow_common.h"
#include "env_common.h"

namespace orbit {
namespace raster {

// What sky_common.h tells whoever wants to count its cases, behind env_common.h's 64 entries (orbit_host_c.h)
enum : uint32_t {
    kSkyCensusEvaluated = 64, // K1: a SKY light evaluated
    kSkyCensusSkipped,        // K1: a SKY light skipped, the environment NULL
    kSkyCensusNdvNegative,    // K3: dot(N, V) < 0
    kSkyCensusNdvZero,        //     == 0
    kSkyCensusNdvOne,         //     == 1
    kSkyCensusNdvNan,         //     NaN
    kSkyCensusNdvOther,       //     any other value
    kSkyCensusRough,          // K3: max(1 - roughness, f0_c) took 1 - roughness
    kSkyCensusF0,             //     took f0_c
    kSkyCensusBadNormal,      // K4: a bad direction
    kSkyCensusBadReflection,  // K5: a bad direction
    kSkyCensusTableLow,       // K6: an index clamped at 0
    kSkyCensusTableHigh,      //     at n - 1
    kSkyCensusTableInside,    //     a tap with neither index clamped
    kSkyCensusAoNull,         // K8: the plane NULL
    kSkyCensusAoBelowOne,     //     ao[p] < 1
    kSkyCensusAoOne,          //     1.0f taken (ao[p] >= 1 or NaN)
    kSkyCensusSkybox,         // K9: a pixel written
    kSkyCensusSkyboxBad,      //     with a bad direction
    kSkyCensusSecond,         // K1: a second SKY light of one walk
    kSkyCensusSize = 96
};

// K1's condition: the environment is given (sky_check: its three images together or not at all) and the mode evaluates lights
ORBIT_RASTER_FN bool sky_env_given(const OrbitFragmentsShadeSky &j) { return j.irradiance != nullptr && j.shadowed.shade.render_mode == 0u; }

// K6: the table under LinearClamp at (u, v) -> (A, B)
ORBIT_RASTER_FN void sky_table_texel(const uint16_t *table, uint32_t n, uint32_t x, uint32_t y, float *ab) {
    uint32_t pair;
    __builtin_memcpy(&pair, __builtin_assume_aligned(table + 2u * ((size_t)y * n + x), 4), 4);
    ab[0] = env_unhalf((uint16_t)(pair & 0xFFFFu)), ab[1] = env_unhalf((uint16_t)(pair >> 16));
}
template <class Census = EnvNoCensus>
ORBIT_RASTER_FN void sky_table(const uint16_t *table, uint32_t n, float u, float v, float *ab, const Census &census = Census()) {
    const float nf = (float)n, sx = u * nf - 0.5f, sy = v * nf - 0.5f;
    const float flx = floorf(sx), fly = floorf(sy), fx = sx - flx, fy = sy - fly, gx = 1.0f - fx, gy = 1.0f - fy;
    const uint32_t x0 = shadow_texel(flx, n), x1 = shadow_texel(flx + 1.0f, n), y0 = shadow_texel(fly, n), y1 = shadow_texel(fly + 1.0f, n);
    census(!(flx >= 0.0f) || !(fly >= 0.0f) ? kSkyCensusTableLow : (flx + 1.0f >= nf || fly + 1.0f >= nf) ? kSkyCensusTableHigh : kSkyCensusTableInside);
    float t00[2], t10[2], t01[2], t11[2];
    sky_table_texel(table, n, x0, y0, t00), sky_table_texel(table, n, x1, y0, t10);
    sky_table_texel(table, n, x0, y1, t01), sky_table_texel(table, n, x1, y1, t11);
    for (int k = 0; k < 2; k++) ab[k] = (t00[k] * gx + t10[k] * fx) * gy + (t01[k] * gx + t11[k] * fx) * fy;
}

// What K adds to a pixel under the walk: the material's roughness, K8's ao and K10's counters
struct SkyPixel {
    float roughness, ao;
    uint32_t evaluations, bad;
};
template <class Census = EnvNoCensus>
ORBIT_RASTER_FN void sky_pixel_begin(const OrbitFragmentsShadeSky &j, float roughness, size_t p, SkyPixel &k, const Census &census = Census()) {
    k.roughness = roughness, k.evaluations = 0u, k.bad = 0u;
    k.ao = 1.0f; // K8
    if (j.ao) {
        k.ao = shade_min(1.0f, j.ao[p]);
        census(j.ao[p] < 1.0f ? kSkyCensusAoBelowOne : kSkyCensusAoOne);
    } else {
        census(kSkyCensusAoNull);
    }
}

// K2-K7 of one SKY light (its lc) at a pixel -> the term; k.bad: E4's bad directions among the two samples.  The two cube
// samples are the two trips of one loop: on the device one body of env_sample serves both, and what it keeps in registers is
// one sample's, not two.  The cube of a trip is built where it is used, from the job's wave-uniform fields: its level
// offsets live in scalar registers for the length of the term only.
template <class Census = EnvNoCensus>
ORBIT_RASTER_FN void sky_light_term(const OrbitFragmentsShadeSky &j, const float *lc, const ShadePixel &px, SkyPixel &k, float *term,
                                    const Census &census = Census()) {
    const float nv = shade_dot(px.N, px.V), two_nv = 2.0f * nv;
    float R[3]; // K2
    for (int i = 0; i < 3; i++) R[i] = px.V[i] - two_nv * px.N[i];
    R[1] = R[1] * -1.0f;
    const float ndv0 = shade_max(nv, 0.0f); // K3
    census(nv < 0.0f ? kSkyCensusNdvNegative : nv == 0.0f ? kSkyCensusNdvZero : nv == 1.0f ? kSkyCensusNdvOne : nv != nv ? kSkyCensusNdvNan : kSkyCensusNdvOther);
    const float x = shade_clamp(1.0f - ndv0, 0.0f, 1.0f), p5 = ((x * x) * (x * x)) * x;
    const float smooth = 1.0f - k.roughness;
    float irr[3] = {0.0f, 0.0f, 0.0f}, refl[3] = {0.0f, 0.0f, 0.0f}, ab[2];
#ifdef __HIP_DEVICE_COMPILE__
#pragma nounroll
#endif
    for (int pass = 0; pass < 2; pass++) { // K4, then K5
        const bool second = pass != 0;
        const EnvCube cube = env_cube(second ? j.prefiltered : j.irradiance, second ? j.prefiltered_size : j.irradiance_size,
                                      second ? j.prefiltered_levels : 1u);
        const float d[3] = {second ? R[0] : px.N[0], second ? R[1] : px.N[1], second ? R[2] : px.N[2]};
        const float lod = second ? k.roughness * (float)(j.prefiltered_levels - 1u) : 0.0f;
        float rgb[3];
        if (!env_sample(cube, d, lod, rgb, census)) {
            k.bad++;
            census(second ? kSkyCensusBadReflection : kSkyCensusBadNormal);
        }
        for (int i = 0; i < 3; i++) {
            if (second) refl[i] = rgb[i];
            else irr[i] = rgb[i];
        }
    }
    sky_table(j.brdf, j.brdf_size, ndv0, k.roughness, ab, census); // K6
    for (int i = 0; i < 3; i++) {
        census(smooth < px.f0[i] ? kSkyCensusF0 : kSkyCensusRough);
        const float kS = px.f0[i] + (shade_max(smooth, px.f0[i]) - px.f0[i]) * p5;
        const float kD = (1.0f - kS) * px.one_minus_metallic;
        const float diffuse = irr[i] * px.albedo[i];
        const float spec = refl[i] * (kS * ab[0] + ab[1]);
        term[i] = ((kD * diffuse + spec) * lc[i]) * k.ao; // K7
    }
}

// K1, then L5, L6 and H9: one light of the walk, shadow_light_checked.  ENV = false: a caller that knows the environment to
// be NULL (a kernel built without K2-K7)
template <bool ENV = true, class Census = EnvNoCensus>
ORBIT_RASTER_FN void sky_pixel_light(const OrbitFragmentsShadeSky &j, const ShadeLight &l, uint32_t x, uint32_t y, ShadePixel &px, ShadowPixel &sp,
                                     SkyPixel &k, const Census &census = Census()) {
    const bool given = ENV && sky_env_given(j);
    if (l.type == kLightSky) census(given ? kSkyCensusEvaluated : kSkyCensusSkipped);
    if (l.type != kLightSky || !given) {
        shadow_pixel_light(j.shadowed, l, x, y, px, sp);
        return;
    }
    float term[3];
    sky_light_term(j, l.lc, px, k, term, census);
    if (k.evaluations != 0u) census(kSkyCensusSecond);
    k.evaluations++;
    for (int i = 0; i < 3; i++) px.sum[i] = px.sum[i] + term[i];
}

// orbit_fragments_shade_sky's tier of shade_common.h's walk.  ENV as sky_pixel_light's; the host mirror's instance carries
// its census, a kernel's carries nothing
struct SkyExtra {
    ShadowPixel sp;
    SkyPixel k;
};
template <bool ENV = true, class Census = EnvNoCensus>
struct SkyTier {
    using Job = OrbitFragmentsShadeSky;
    using Extra = SkyExtra;
    Census census;
    ORBIT_RASTER_FN static const OrbitFragmentsShade &base(const Job &j) { return j.shadowed.shade; }
    ORBIT_RASTER_FN static void reset(Extra &e) {
        shadow_pixel_begin(1.0f, e.sp);
        e.k.roughness = 0.0f, e.k.ao = 1.0f, e.k.evaluations = 0u, e.k.bad = 0u;
    }
    ORBIT_RASTER_FN void begin(const Job &j, const OrbitMaterialData &m, const float *wp, size_t p, Extra &e) const {
        e.sp.w = wp[3];
        if (ENV && sky_env_given(j)) sky_pixel_begin(j, m.roughness_factor, p, e.k, census); // (ao has no other reader)
    }
    ORBIT_RASTER_FN static bool light_checked(const Job &j, uint32_t type, uint32_t shadow) { return shadow_light_checked(j.shadowed, type, shadow); }
    ORBIT_RASTER_FN void light(const Job &j, const ShadeLight &l, uint32_t x, uint32_t y, ShadePixel &px, Extra &e) const {
        sky_pixel_light<ENV>(j, l, x, y, px, e.sp, e.k, census);
    }
    ORBIT_RASTER_FN static bool stale(const Extra &e) { return e.sp.stale; }
    ORBIT_RASTER_FN static void end(Extra &e) { finite_or_zero(e.sp.factor); }
};

// K9 of uncovered pixel (x, y) -> the direction was good
template <class Census = EnvNoCensus>
ORBIT_RASTER_FN bool sky_box_pixel(const OrbitFragmentsShadeSky &j, uint32_t x, uint32_t y, float *color, const Census &census = Census()) {
    const EnvCube sky = env_cube(j.sky, j.sky_size, j.sky_levels); // (built where it is used, as sky_light_term's)
    const OrbitFragmentsShade &b = j.shadowed.shade;
    const float cx = (2.0f * ((float)x + 0.5f)) / (float)b.width - 1.0f, cy = 1.0f - (2.0f * ((float)y + 0.5f)) / (float)b.height;
    float d[3];
    for (int i = 0; i < 3; i++) d[i] = (cx * j.sky_x[i] + cy * j.sky_y[i]) + j.sky_z[i];
    shade_normalize(d);
    const bool good = env_sample(sky, d, j.skybox_lod, color, census);
    for (int i = 0; i < 3; i++) finite_or_zero(color[i]); // L8
    color[3] = 1.0f;
    census(good ? kSkyCensusSkybox : kSkyCensusSkyboxBad);
    return good;
}
// K9 applies
ORBIT_RASTER_FN bool sky_box_given(const OrbitFragmentsShadeSky &j) { return j.sky != nullptr && j.shadowed.shade.render_mode == 0u; }

// the texels of a cube in E0's layout
inline uint64_t sky_cube_texels(uint32_t size, uint32_t levels) {
    uint64_t texels = 0u;
    for (uint32_t m = 0; m < levels; m++) texels += 6ull * env_level_size(size, m) * env_level_size(size, m);
    return texels;
}

// The argument errors of orbit_fragments_shade_sky, the base job's and the shadow fields' included: nullptr, or what is wrong
inline const char *sky_check(const OrbitFragmentsShadeSky &js) {
    const OrbitFragmentsShadeShadowed &j = js.shadowed;
    const OrbitFragmentsShade &b = j.shade;
    const uint32_t known = ORBIT_SHADE_CLEAR | ORBIT_SHADE_FORCE_PER_LANE | ORBIT_SHADE_FORCE_STAGED;
    if (b.flags & ~known) return "unknown flags";
    if ((b.flags & ORBIT_SHADE_FORCE_PER_LANE) && (b.flags & ORBIT_SHADE_FORCE_STAGED)) return "ORBIT_SHADE_FORCE_PER_LANE and ORBIT_SHADE_FORCE_STAGED together";
    if (b.render_mode != 0u && b.render_mode != 8u) return "render_mode (0 or 8)";
    if (b.width == 0 || b.height == 0 || b.width > ORBIT_RASTER_MAX_DIM || b.height > ORBIT_RASTER_MAX_DIM) return "target size (1..32768 each)";
    if (b.cluster_count[0] == 0 || b.cluster_count[1] == 0 || b.cluster_count[2] == 0 || b.tile_size_px == 0) return "a zero in cluster_count or tile_size_px";
    if (b.cluster_count[2] > 32u) return "cluster_count[2] > 32";
    if ((uint64_t)b.cluster_count[0] * b.cluster_count[1] > (1ull << 31) / b.cluster_count[2]) return "clusters > 2^31";
    if ((b.flags & ORBIT_SHADE_FORCE_STAGED) && b.tile_size_px % 8u != 0u) return "ORBIT_SHADE_FORCE_STAGED needs tile_size_px % 8 == 0";
    if (!b.visibility || !b.world_pos || !b.normal || !b.material || !b.materials || !b.lights || !b.cluster_offset_image || !b.light_index_buffer ||
        !b.color)
        return "NULL buffer";
    if (j.shadow_count > 0u) {
        if (!j.shadows || !j.shadow_maps) return "shadow_count > 0 with shadows or shadow_maps NULL";
        if (j.shadow_resolution == 0u || j.shadow_resolution > ORBIT_RASTER_MAX_DIM) return "shadow_resolution (1..32768)";
        if ((uint64_t)j.shadow_map_count * j.shadow_resolution * j.shadow_resolution > (1ull << 31)) return "shadow maps > 2^31 floats";
    }
    const bool any = js.irradiance || js.prefiltered || js.brdf, all = js.irradiance && js.prefiltered && js.brdf;
    if (any && !all) return "the environment given in part: irradiance, prefiltered and brdf go together";
    if (all) {
        if (js.irradiance_size == 0u || js.irradiance_size > ORBIT_ENV_MAX_SIZE) return "irradiance_size (1..4096)";
        if (js.prefiltered_size == 0u || js.prefiltered_size > ORBIT_ENV_MAX_SIZE) return "prefiltered_size (1..4096)";
        if (js.prefiltered_levels == 0u || js.prefiltered_levels > ORBIT_ENV_MAX_LEVELS) return "prefiltered_levels (1..13)";
        if (js.brdf_size == 0u || js.brdf_size > ORBIT_ENV_MAX_SIZE) return "brdf_size (1..4096)";
    }
    if (js.sky) {
        if (js.sky_size == 0u || js.sky_size > ORBIT_ENV_MAX_SIZE) return "sky_size (1..4096)";
        if (js.sky_levels == 0u || js.sky_levels > ORBIT_ENV_MAX_LEVELS) return "sky_levels (1..13)";
        if (!(fabsf(js.skybox_lod) < INFINITY)) return "skybox_lod is not finite";
    }
    const size_t pixels = (size_t)b.width * b.height;
    const uint64_t clusters = (uint64_t)b.cluster_count[0] * b.cluster_count[1] * b.cluster_count[2];
    const void *const inputs[15] = {b.visibility, b.world_pos, b.normal,   b.material,     b.materials, b.lights, b.cluster_offset_image, b.light_index_buffer,
                                    j.shadows,    j.shadow_maps, js.irradiance, js.prefiltered, js.brdf,     js.sky,   js.ao};
    const uint64_t input_bytes[15] = {8ull * pixels,
                                      16ull * pixels,
                                      12ull * pixels,
                                      4ull * pixels,
                                      80ull * b.material_count,
                                      64ull * b.light_count,
                                      8ull * clusters,
                                      ORBIT_LIGHT_INDEX_HEADER + 4ull * b.index_capacity,
                                      288ull * j.shadow_count,
                                      4ull * j.shadow_map_count * j.shadow_resolution * j.shadow_resolution,
                                      all ? 8ull * sky_cube_texels(js.irradiance_size, 1u) : 0u,
                                      all ? 8ull * sky_cube_texels(js.prefiltered_size, js.prefiltered_levels) : 0u,
                                      all ? 4ull * js.brdf_size * js.brdf_size : 0u,
                                      js.sky ? 8ull * sky_cube_texels(js.sky_size, js.sky_levels) : 0u,
                                      4ull * pixels};
    const void *const outputs[7] = {b.color, b.lights_walked, b.stats, j.shadow_factor, j.cascade, j.shadow_stats, js.sky_stats};
    const uint64_t output_bytes[7] = {16ull * pixels, 4ull * pixels,           sizeof(OrbitShadeStats), 4ull * pixels,
                                      4ull * pixels,  sizeof(OrbitShadowStats), sizeof(OrbitSkyStats)};
    uintptr_t low_bits = 0;
    for (const void *in : inputs) low_bits |= (uintptr_t)in;
    for (const void *out : outputs) low_bits |= (uintptr_t)out;
    if ((((uintptr_t)b.visibility | (uintptr_t)b.cluster_offset_image) & 7u) || (((uintptr_t)b.materials | (uintptr_t)b.lights | (uintptr_t)j.shadows) & 15u) ||
        (low_bits & 3u))
        return "alignment: visibility and cluster_offset_image 8 B, materials, lights and shadows 16 B, every other buffer 4 B";
    if (((uintptr_t)js.irradiance | (uintptr_t)js.prefiltered | (uintptr_t)js.sky | (uintptr_t)js.sky_stats) & 7u)
        return "alignment: irradiance, prefiltered, sky and sky_stats 8 B";
    for (int o = 0; o < 7; o++)
        for (int i = 0; i < 15; i++)
            if (outputs[o] && (outputs[o] == inputs[i] || env_ranges_overlap(outputs[o], output_bytes[o], inputs[i], input_bytes[i])))
                return "an output shares bytes with an input";
    return nullptr;
}

} // namespace raster
} // namespace orbit
