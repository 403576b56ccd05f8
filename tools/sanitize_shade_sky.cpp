// sanitize_shade_sky.cpp — the host mirror of orbit_fragments_shade_sky (orbit_amd/host/orbit_raster.cpp over
// csrc/sky_common.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host program: targets of 1 x
// 1, 8 x 8 and 9 x 7 with lists that hold the sky light first, last and twice beside a shadowed sun and point lights;
// irradiance cubes of 1 to 8, prefiltered cubes of 1 to 16 with 1, 2 and 5 levels, tables of 1 to 17, sky cubes of 1 to 16
// with their full chains, NaN and inf halves among the texels; normals and positions that put N and R on face centres,
// edges and corners, zero and non-finite ones; roughness from 0 to NaN; an ao plane with values from -1 to NaN; bases
// whose rays hit edges and corners and a zero basis; lods from 0 to beyond the chain — every plane, table, cube and counter
// block in a heap buffer that ENDS at its last legal byte, so a tap or a pixel past the end is a heap overflow; each optional
// input alone; then the jobs the call must refuse.  Host code only; nothing of it runs on a device or inside Python.  From
// the repository root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iorbit_amd/host \
//       tools/sanitize_shade_sky.cpp orbit_amd/host/orbit_raster.cpp -o /tmp/sanitize_shade_sky && /tmp/sanitize_shade_sky
// Exit status 0, one line of counters per case and the number of refused jobs is a clean run.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../orbit_amd/csrc/sky_common.h"
#include "orbit_host.hpp"
#include "orbit_raster.hpp"
using namespace orbit;

template <class T>
static T *ending(size_t count) { // a heap block of exactly count elements (at least 16 bytes' worth of alignment from malloc)
    T *p = (T *)std::malloc(count ? count * sizeof(T) : 1);
    std::memset((void *)p, 0, count ? count * sizeof(T) : 1);
    return p;
}

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t &s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

static uint16_t *make_cube(uint32_t size, uint32_t levels, uint32_t seed, bool hostile) {
    const uint64_t texels = raster::sky_cube_texels(size, levels);
    uint16_t *c = ending<uint16_t>(texels * 4);
    const uint16_t odd[] = {0x7E00u, 0x7C00u, 0xFC00u, 0x7BFFu, 0x0001u, 0x8000u}; // NaN, +inf, -inf, 65504, a denormal, -0
    for (uint64_t i = 0; i < texels * 4; i++) {
        bool nonfinite = false;
        c[i] = (i & 3u) == 3u ? 0x3C00u : raster::env_half(unit(seed) * 4.0f, nonfinite);
        if (hostile && i % 7u == 0u) c[i] = odd[(i / 7u) % 6u];
    }
    return c;
}

static uint64_t refused = 0;
static void expect_refused(const OrbitFragmentsShadeSky &j, const char *what) {
    try {
        raster::fragments_shade_sky(j, nullptr);
    } catch (const Panic &) {
        refused++;
        return;
    }
    std::fprintf(stderr, "not refused: %s\n", what);
    std::exit(1);
}

struct Case {
    uint32_t w, h, tile, irr, pre, levels, table, sky;
    bool hostile;
    float lod;
    int basis;
};

int main() {
    const Case cases[] = {{1, 1, 8, 1, 1, 1, 1, 1, false, 0.0f, 0},  {8, 8, 8, 2, 2, 2, 2, 2, false, 0.5f, 1},  {9, 7, 4, 5, 5, 5, 16, 16, true, 20.0f, 2},
                          {8, 8, 4, 8, 16, 5, 17, 16, false, 1.25f, 3}, {9, 7, 8, 8, 16, 1, 16, 1, true, NAN, 0}, {8, 8, 8, 5, 1, 5, 2, 2, false, -1.0f, 1}};
    const float bases[4][9] = {{1, 0, 0, 0, 1, 0, 0, 0, -1}, {0, 0, 1, 0, 0, 0, 1, 1, 0}, {0, 0, 8, 0, 0, 0, 1, 1, 0}, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
    const float roughness[] = {0.0f, 0.25f, 0.3f, 1.0f, 1.5f, NAN, INFINITY, -1.0f, 3.0e38f};
    const float aos[] = {0.0f, 0.5f, 1.0f, 2.0f, -1.0f, NAN, INFINITY};
    const float parts[] = {0.0f, 1.0f, -1.0f, 0.999f, 1e30f, 1e-30f, NAN, INFINITY, 0.5f};
    for (const Case &c : cases) {
        uint32_t seed = 777u + c.w * 31u + c.irr;
        const size_t pixels = (size_t)c.w * c.h;
        const uint32_t cx = (c.w + c.tile - 1u) / c.tile, cy = (c.h + c.tile - 1u) / c.tile, cz = 4u;
        uint64_t *vis = ending<uint64_t>(pixels);
        float *wp = ending<float>(pixels * 4), *nrm = ending<float>(pixels * 3), *ao = ending<float>(pixels);
        uint32_t *material = ending<uint32_t>(pixels);
        const uint32_t n_materials = 9u, n_lights = 6u;
        OrbitMaterialData *materials = ending<OrbitMaterialData>(n_materials);
        OrbitLightData *lights = ending<OrbitLightData>(n_lights);
        for (uint32_t i = 0; i < n_materials; i++) {
            for (int k = 0; k < 4; k++) materials[i].base_color[k] = i == 1u ? 0.0f : unit(seed) * 1.5f;
            materials[i].metallic_factor = 0.5f * (float)(i % 3u), materials[i].roughness_factor = roughness[i];
            materials[i].base_texture_index = materials[i].normal_texture_index = materials[i].metallic_roughness_texture_index = 0xFFFFFFFFu;
            materials[i].occlusion_texture_index = materials[i].emissive_texture_index = 0xFFFFFFFFu;
        }
        for (uint32_t i = 0; i < n_lights; i++) {
            lights[i].light_type = i < 2u ? 0u : i == 2u ? 1u : 2u; // two sky lights, a shadowed sun, points
            lights[i].shadow_data_index = i == 2u ? 0u : 0xFFFFFFFFu;
            for (int k = 0; k < 3; k++) lights[i].color[k] = unit(seed), lights[i].position[k] = unit(seed) * 8.0f - 4.0f;
            lights[i].direction[0] = 0.0f, lights[i].direction[1] = 1.0f, lights[i].direction[2] = 0.0f;
            lights[i].intensity = i == 1u ? 0.0f : 3.0f, lights[i].inner_radius = 0.1f, lights[i].outer_radius = 20.0f;
        }
        for (size_t p = 0; p < pixels; p++) {
            const bool covered = p % 5u != 3u;
            const float depth = (p & 1u) ? 0.02f : 0.004f;
            uint32_t bits;
            std::memcpy(&bits, &depth, 4);
            vis[p] = covered ? ((uint64_t)bits << 32) | ((p + 1u) << 8) | 1u : 0u;
            for (int k = 0; k < 3; k++) wp[4 * p + k] = p % 11u == 10u ? 0.0f : unit(seed) * 6.0f - 3.0f;
            wp[4 * p + 3] = 1.0f;
            for (int k = 0; k < 3; k++) nrm[3 * p + k] = parts[(p / (k == 0 ? 1u : k == 1 ? 9u : 81u) + (uint32_t)k) % 9u];
            if (p % 13u >= 11u) nrm[3 * p] = nrm[3 * p + 1] = 1.0f, nrm[3 * p + 2] = p % 13u == 12u ? 1.0f : 0.0f; // a corner, an edge
            material[p] = (uint32_t)(p % n_materials), ao[p] = aos[p % 7u];
        }
        // every cluster walks one of three lists
        const uint32_t clusters = cx * cy * cz, walks[3][5] = {{0, 3, 2, 4, 0}, {5, 2, 1, 0, 0}, {0, 0, 0, 0, 0}}, lengths[3] = {5, 4, 2};
        uint32_t *image = ending<uint32_t>(2u * clusters), *indices = ending<uint32_t>(1u + 5u * clusters);
        uint32_t at = 0;
        for (uint32_t k = 0; k < clusters; k++) {
            image[2 * k] = at, image[2 * k + 1] = lengths[k % 3u];
            for (uint32_t i = 0; i < lengths[k % 3u]; i++) indices[1u + at++] = walks[k % 3u][i];
        }
        indices[0] = at;
        OrbitShadowData *shadows = ending<OrbitShadowData>(1);
        for (int m = 0; m < 4; m++) {
            float *M = shadows->light_projection_matrices[m];
            M[0] = M[5] = 0.2f, M[10] = 0.1f, M[14] = 0.5f, M[15] = 1.0f;
            shadows->shadow_map_world_sizes[m] = 1.0f, shadows->shadow_map_indices[m] = (uint32_t)m % 2u;
        }
        const uint32_t res = 3u;
        float *maps = ending<float>(2u * res * res);
        for (uint32_t i = 0; i < 2u * res * res; i++) maps[i] = unit(seed);
        uint16_t *irr = make_cube(c.irr, 1u, seed + 1u, c.hostile), *pre = make_cube(c.pre, c.levels, seed + 2u, c.hostile);
        uint32_t sky_levels = 0u;
        for (uint32_t v = c.sky; v != 0u; v >>= 1) sky_levels++;
        uint16_t *sky = make_cube(c.sky, sky_levels, seed + 3u, c.hostile);
        uint16_t *table = ending<uint16_t>((size_t)c.table * c.table * 2);
        for (size_t i = 0; i < (size_t)c.table * c.table * 2; i++) {
            bool nonfinite = false;
            table[i] = c.hostile && i % 5u == 0u ? 0x7E00u : raster::env_half(unit(seed), nonfinite);
        }
        float *color = ending<float>(pixels * 4), *factor = ending<float>(pixels);
        uint32_t *walked = ending<uint32_t>(pixels), *cascade = ending<uint32_t>(pixels);
        OrbitShadeStats *stats = ending<OrbitShadeStats>(1);
        OrbitShadowStats *shadow_stats = ending<OrbitShadowStats>(1);
        OrbitSkyStats *sky_stats = ending<OrbitSkyStats>(1);
        OrbitFragmentsShadeSky j{};
        OrbitFragmentsShadeShadowed &s = j.shadowed;
        OrbitFragmentsShade &b = s.shade;
        b.visibility = vis, b.world_pos = wp, b.normal = nrm, b.material = material, b.materials = materials, b.lights = lights;
        b.cluster_offset_image = image, b.light_index_buffer = indices, b.color = color, b.lights_walked = walked, b.stats = stats;
        b.material_count = n_materials, b.light_count = n_lights, b.index_capacity = at;
        b.cluster_count[0] = cx, b.cluster_count[1] = cy, b.cluster_count[2] = cz, b.tile_size_px = c.tile;
        b.z_scale = 1.0f, b.z_bias = 0.0f, b.luminance_cutoff = 0.01f, b.z_near = 0.01f;
        b.view_pos[0] = 0.0f, b.view_pos[1] = 0.0f, b.view_pos[2] = 0.0f, b.render_mode = 0u, b.width = c.w, b.height = c.h, b.flags = ORBIT_SHADE_CLEAR;
        s.shadows = shadows, s.shadow_maps = maps, s.shadow_factor = factor, s.cascade = cascade, s.shadow_stats = shadow_stats;
        s.shadow_count = 1u, s.shadow_index_base = 0u, s.shadow_map_count = 2u, s.shadow_resolution = res;
        s.blocker_search_radius = 0.3f, s.normal_bias_scale = 2.0f, s.oriented_bias = -0.02f;
        j.irradiance = irr, j.prefiltered = pre, j.brdf = table, j.sky = sky, j.ao = ao, j.sky_stats = sky_stats;
        j.irradiance_size = c.irr, j.prefiltered_size = c.pre, j.prefiltered_levels = c.levels, j.brdf_size = c.table;
        j.sky_size = c.sky, j.sky_levels = sky_levels, j.skybox_lod = std::isnan(c.lod) ? 0.0f : c.lod;
        std::memcpy(j.sky_x, bases[c.basis], 12), std::memcpy(j.sky_y, bases[c.basis] + 3, 12), std::memcpy(j.sky_z, bases[c.basis] + 6, 12);
        uint64_t census[raster::kSkyCensusSize] = {0};
        int32_t status = 0;
        raster::fragments_shade_sky(j, &status, census);
        const OrbitSkyStats whole = *sky_stats;
        uint64_t corner_taps = 0;
        for (uint32_t i = 30u; i < 54u; i++) corner_taps += census[i];
        for (size_t i = 0; i < pixels * 4; i++)
            if (!(std::fabs(color[i]) < INFINITY)) return std::fprintf(stderr, "a non-finite colour float\n"), 1;
        // each optional input alone, the heat map, no optional output
        OrbitFragmentsShadeSky k = j;
        k.sky = nullptr, raster::fragments_shade_sky(k, &status), k = j;
        k.irradiance = k.prefiltered = k.brdf = nullptr, raster::fragments_shade_sky(k, &status);
        k.sky = nullptr, k.ao = nullptr, raster::fragments_shade_sky(k, &status), k = j;
        k.shadowed.shade.render_mode = 8u, raster::fragments_shade_sky(k, &status), k = j;
        k.ao = nullptr, k.sky_stats = nullptr, k.shadowed.shade.stats = nullptr, k.shadowed.shade.lights_walked = nullptr, k.shadowed.shadow_factor = nullptr;
        k.shadowed.cascade = nullptr, k.shadowed.shadow_stats = nullptr, k.shadowed.shade.flags = 0u, raster::fragments_shade_sky(k, &status);
        std::printf("%u x %u tile %u, irradiance %u prefiltered %u x %u table %u sky %u: sky evaluations %u over %u pixels, skybox %u, bad directions %llu, "
                    "corner taps %llu, status %d\n", c.w, c.h, c.tile, c.irr, c.pre, c.levels, c.table, c.sky, whole.sky_evaluations, whole.sky_lit_pixels,
                    whole.skybox_pixels, (unsigned long long)whole.bad_directions, (unsigned long long)corner_taps, status);
        // the refused jobs, on this case's buffers
        OrbitFragmentsShadeSky r = j;
        r.brdf = nullptr, expect_refused(r, "the environment in part"), r = j;
        r.irradiance = nullptr, expect_refused(r, "the environment in part"), r = j;
        r.irradiance_size = 0u, expect_refused(r, "irradiance_size 0"), r = j;
        r.prefiltered_size = 4097u, expect_refused(r, "prefiltered_size above 4096"), r = j;
        r.prefiltered_levels = 0u, expect_refused(r, "prefiltered_levels 0"), r = j;
        r.prefiltered_levels = 14u, expect_refused(r, "prefiltered_levels 14"), r = j;
        r.brdf_size = 0u, expect_refused(r, "brdf_size 0"), r = j;
        r.sky_size = 0u, expect_refused(r, "sky_size 0"), r = j;
        r.sky_levels = 14u, expect_refused(r, "sky_levels 14"), r = j;
        r.skybox_lod = NAN, expect_refused(r, "skybox_lod NaN"), r = j;
        r.skybox_lod = INFINITY, expect_refused(r, "skybox_lod inf"), r = j;
        r.irradiance = irr + 2, expect_refused(r, "irradiance misaligned"), r = j;
        r.sky = sky + 1, expect_refused(r, "sky misaligned"), r = j;
        r.brdf = table + 1, expect_refused(r, "table misaligned"), r = j;
        r.sky_stats = (OrbitSkyStats *)((uint8_t *)sky_stats + 4), expect_refused(r, "sky_stats misaligned"), r = j;
        r.ao = (const float *)((const uint8_t *)ao + 2), expect_refused(r, "ao misaligned"), r = j;
        r.ao = color, expect_refused(r, "ao is color"), r = j;
        r.sky_stats = (OrbitSkyStats *)irr, expect_refused(r, "sky_stats is irradiance"), r = j;
        r.shadowed.shade.color = (float *)(void *)(pre + 4 * (raster::sky_cube_texels(c.pre, c.levels) - 1u)), expect_refused(r, "color inside the prefiltered cube's last texel"), r = j;
        r.shadowed.shade.render_mode = 1u, expect_refused(r, "render_mode 1"), r = j;
        r.shadowed.shade.width = 0u, expect_refused(r, "width 0"), r = j;
        r.shadowed.shadow_resolution = 0u, expect_refused(r, "shadow_resolution 0");
        std::free(vis), std::free(wp), std::free(nrm), std::free(ao), std::free(material), std::free(materials), std::free(lights), std::free(image);
        std::free(indices), std::free(shadows), std::free(maps), std::free(irr), std::free(pre), std::free(sky), std::free(table), std::free(color);
        std::free(factor), std::free(walked), std::free(cascade), std::free(stats), std::free(shadow_stats), std::free(sky_stats);
    }
    std::printf("refused %llu jobs\n", (unsigned long long)refused);
    return 0;
}
