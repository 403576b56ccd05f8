// orbit_env_map.cpp — see orbit_env_map.hpp.
#include "orbit_env_map.hpp"

#include <cmath>
#include <cstring>
#include <string>

#include "../csrc/env_common.h"
#include "orbit_host.hpp"

namespace orbit {
namespace raster {

namespace {

void store_texel(uint16_t *dst, size_t texel, const EnvTexel &t) { std::memcpy(dst + 4u * texel, &t, 8); }

struct Counting { // the sampler's census hook: counts into the tests' block, or nowhere
    uint64_t *census;
    void operator()(uint32_t index) const {
        if (census) census[index]++;
    }
};

} // namespace

void env_map(const OrbitEnvMap &j, uint64_t *census) {
    if (const char *wrong = env_map_check(j)) throw Panic(std::string("env_map: ") + wrong);
    OrbitEnvMapStats st{};
    const uint32_t sky_levels = j.sky ? env_full_levels(j.sky_size) : 0u;
    const EnvCube sky = env_cube(j.sky, j.sky_size, sky_levels ? sky_levels : 1u);
    const Counting counting{census};
    if (j.equirect) {
        const uint32_t n = j.sky_size;
        for (uint32_t face = 0; face < 6u; face++)
            for (uint32_t py = 0; py < n; py++)
                for (uint32_t px = 0; px < n; px++) {
                    float rgb[3];
                    env_equirect_texel(j.equirect, j.equirect_w, j.equirect_h, face, px, py, n, rgb);
                    EnvTexel t;
                    if (env_store_rgb(rgb, t)) st.sky_nonfinite++;
                    store_texel(j.sky, ((size_t)face * n + py) * n + px, t);
                }
        for (uint32_t m = 1; m < sky_levels; m++) {
            const uint32_t d = j.sky_size >> m;
            const uint16_t *src = j.sky + 4u * (size_t)sky.offset[m - 1u];
            uint16_t *dst = j.sky + 4u * (size_t)sky.offset[m];
            for (uint32_t face = 0; face < 6u; face++)
                for (uint32_t y = 0; y < d; y++)
                    for (uint32_t x = 0; x < d; x++) {
                        EnvTexel t;
                        if (env_mip_texel(src + 4u * ((size_t)face * (2u * d) * (2u * d)), 2u * d, x, y, t)) st.sky_nonfinite++;
                        store_texel(dst, ((size_t)face * d + y) * d + x, t);
                    }
        }
    }
    if (j.irradiance) {
        const uint32_t n = j.irradiance_size;
        const float lod = env_irradiance_lod(j.sky_size, n);
        for (uint32_t face = 0; face < 6u; face++)
            for (uint32_t py = 0; py < n; py++)
                for (uint32_t px = 0; px < n; px++) {
                    float rgb[3];
                    uint64_t bad = 0u;
                    env_irradiance_texel(sky, lod, j.sample_delta, face, px, py, n, rgb, bad, counting);
                    EnvTexel t;
                    if (env_store_rgb(rgb, t)) st.irradiance_nonfinite++;
                    store_texel(j.irradiance, ((size_t)face * n + py) * n + px, t);
                    st.bad_directions += bad;
                    if (census && bad != 0u) census[59]++;
                }
    }
    if (j.prefiltered) {
        const EnvCube out = env_cube(j.prefiltered, j.prefiltered_size, j.prefiltered_levels);
        for (uint32_t m = 0; m < j.prefiltered_levels; m++) {
            const uint32_t n = env_level_size(j.prefiltered_size, m);
            const EnvPrefilterLevel level = env_prefilter_level(m, j.prefiltered_levels, j.sample_count, j.sky_size);
            uint16_t *dst = j.prefiltered + 4u * (size_t)out.offset[m];
            for (uint32_t face = 0; face < 6u; face++)
                for (uint32_t py = 0; py < n; py++)
                    for (uint32_t px = 0; px < n; px++) {
                        EnvPrefilterTexel t;
                        env_prefilter_begin(face, px, py, n, t);
                        for (uint32_t i = 0; i < j.sample_count; i++) {
                            float phi0, cos_theta, sin_theta;
                            env_ggx_entry(i, j.sample_count, level.roughness, phi0, cos_theta, sin_theta);
                            const uint32_t r = env_prefilter_sample(sky, level, phi0, cos_theta, sin_theta, t, counting);
                            if (r == 2u) st.bad_directions++;
                            if (census && r == 0u) census[56]++;
                        }
                        float rgb[3];
                        env_prefilter_end(t, rgb);
                        EnvTexel texel;
                        if (env_store_rgb(rgb, texel)) st.prefiltered_nonfinite++;
                        store_texel(dst, ((size_t)face * n + py) * n + px, texel);
                        if (census) {
                            census[t.z_up ? 54 : 55]++;
                            if (level.roughness == 0.0f) census[57]++;
                            if (t.weight == 0.0f) census[58]++;
                        }
                    }
        }
    }
    if (j.brdf) {
        const uint32_t n = j.brdf_size;
        for (uint32_t y = 0; y < n; y++)
            for (uint32_t x = 0; x < n; x++) {
                float ab[2];
                env_brdf_texel(x, y, n, j.brdf_sample_count, ab);
                bool nonfinite = false;
                const uint16_t pair[2] = {env_half(ab[0], nonfinite), env_half(ab[1], nonfinite)};
                std::memcpy(j.brdf + 2u * ((size_t)y * n + x), pair, 4);
                if (nonfinite) st.brdf_nonfinite++;
            }
    }
    if (j.stats) *j.stats = st;
}

void env_sample_job(const OrbitEnvSample &j, uint64_t *census) {
    if (const char *wrong = env_sample_check(j)) throw Panic(std::string("env_sample: ") + wrong);
    const EnvCube cube = env_cube(j.cube, j.size, j.levels);
    const Counting counting{census};
    uint64_t bad = 0u;
    for (uint32_t i = 0; i < j.n; i++)
        if (!env_sample(cube, j.directions + 3u * (size_t)i, j.lods[i], j.rgb + 3u * (size_t)i, counting)) bad++;
    if (j.bad_directions) *j.bad_directions = bad;
}

void env_prefilter_texels(const OrbitEnvMap &j, uint32_t m, const uint32_t *texels, uint32_t count, uint16_t *out) {
    // `out` holds `count` texels, not a cube: the fields this reads are checked here, not by env_map_check's ranges
    if (!j.sky || ((uintptr_t)j.sky & 7u) || !env_power_of_two(j.sky_size) || j.sky_size > ORBIT_ENV_MAX_SIZE) throw Panic("env_prefilter_texels: sky cube");
    if (j.prefiltered_size == 0u || j.prefiltered_size > ORBIT_ENV_MAX_SIZE || j.prefiltered_levels == 0u || j.prefiltered_levels > ORBIT_ENV_MAX_LEVELS ||
        m >= j.prefiltered_levels || j.sample_count == 0u || j.sample_count > ORBIT_ENV_MAX_SAMPLES)
        throw Panic("env_prefilter_texels: prefiltered size, levels, level or sample_count");
    const EnvCube sky = env_cube(j.sky, j.sky_size, env_full_levels(j.sky_size));
    const uint32_t n = env_level_size(j.prefiltered_size, m);
    const EnvPrefilterLevel level = env_prefilter_level(m, j.prefiltered_levels, j.sample_count, j.sky_size);
    for (uint32_t k = 0; k < count; k++) {
        if (texels[k] >= 6u * n * n) throw Panic("env_prefilter_texels: a texel beyond the level");
        EnvPrefilterTexel t;
        env_prefilter_begin(texels[k] / (n * n), texels[k] % n, (texels[k] / n) % n, n, t);
        for (uint32_t i = 0; i < j.sample_count; i++) {
            float phi0, cos_theta, sin_theta;
            env_ggx_entry(i, j.sample_count, level.roughness, phi0, cos_theta, sin_theta);
            env_prefilter_sample(sky, level, phi0, cos_theta, sin_theta, t);
        }
        float rgb[3];
        env_prefilter_end(t, rgb);
        EnvTexel texel;
        env_store_rgb(rgb, texel);
        store_texel(out, k, texel);
    }
}

void env_direction(uint32_t face, uint32_t px, uint32_t py, uint32_t n, float *out) { env_texel_direction(face, px, py, n, out); }
void env_routines(uint32_t which, const float *a, const float *b, uint64_t n, float *out) {
    for (uint64_t i = 0; i < n; i++) {
        float s, c;
        switch (which) {
        case 0: out[i] = env_atan2c(a[i], b[i]); break;
        case 1: out[i] = env_asinc(a[i]); break;
        case 4: { // E0: the stored half, back as a float; NaN where the value was not finite (no stored half is NaN)
            bool nonfinite = false;
            const uint16_t h = env_half(a[i], nonfinite);
            out[i] = nonfinite ? NAN : env_unhalf(h);
            break;
        }
        default:
            shadow_sincos(a[i], s, c);
            out[i] = which == 2u ? s : c;
        }
    }
}

} // namespace raster
} // namespace orbit
