// sanitize_fragments_shade_shadowed.cpp — the host mirror of orbit_fragments_shade_shadowed (orbit_amd/host/orbit_raster.cpp
// over csrc/shade_common.h and csrc/shadow_common.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
// host program: a 19 x 9 target of hand-built planes over a 3 x 2 x 1 cluster grid of 8-px tiles whose every list walks a
// point light and two shadowed suns, with the shadow rows and the maps (2 maps of 5 x 5 floats) each in a heap buffer that
// ENDS at its last legal byte, so a read past a row or a map is a heap overflow.  The cascade's matrix maps the pixels' x
// and z onto uv in [-0.2, 1.2]^2 and the search radius is wide, so taps leave the map on all four sides and clamp at every
// edge.  First clean, then tampered: a sun whose row is shadow_count, a sun whose index lies below shadow_index_base, a
// row whose map index is shadow_map_count.  Both render modes.  Host code only; nothing of it runs on a device or inside
// Python.  From the repository root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iorbit_amd/host tools/sanitize_fragments_shade_shadowed.cpp orbit_amd/host/orbit_raster.cpp \
//       -o /tmp/sanitize_fragments_shade_shadowed && /tmp/sanitize_fragments_shade_shadowed
// Exit status 0 and four lines of counters is a clean run.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "orbit_raster.hpp"
#include "orbit_host.hpp"
using namespace orbit;
int main() {
    const uint32_t W = 19, H = 9, CX = 3, CY = 2, MATERIALS = 2, LIGHTS = 3, ROWS = 2, MAPS = 2, RES = 5, BASE = 640;
    const size_t clusters = CX * CY, capacity = clusters * 3;
    OrbitMaterialData *materials = (OrbitMaterialData *)std::malloc(MATERIALS * sizeof(OrbitMaterialData));
    OrbitLightData *lights = (OrbitLightData *)std::malloc(LIGHTS * sizeof(OrbitLightData));
    OrbitShadowData *rows = (OrbitShadowData *)std::aligned_alloc(16, ROWS * sizeof(OrbitShadowData)); // 576 B: ends at its last byte
    float *maps = (float *)std::malloc(MAPS * RES * RES * sizeof(float));
    uint32_t *image = (uint32_t *)std::malloc(clusters * 8), *list = (uint32_t *)std::malloc(4 + capacity * 4);
    std::memset(materials, 0, MATERIALS * sizeof(OrbitMaterialData)), std::memset(lights, 0, LIGHTS * sizeof(OrbitLightData));
    std::memset(rows, 0, ROWS * sizeof(OrbitShadowData));
    for (uint32_t m = 0; m < MATERIALS; m++) {
        OrbitMaterialData &r = materials[m];
        r.base_color[0] = 0.8f, r.base_color[1] = 0.5f + 0.1f * (float)m, r.base_color[2] = 0.2f, r.base_color[3] = 1.0f;
        r.metallic_factor = 0.5f * (float)m, r.roughness_factor = 1.0f - 0.5f * (float)m;
        r.base_texture_index = r.normal_texture_index = r.metallic_roughness_texture_index = 0xFFFFFFFFu;
        r.occlusion_texture_index = r.emissive_texture_index = 0xFFFFFFFFu;
    }
    for (uint32_t l = 0; l < LIGHTS; l++) {
        OrbitLightData &r = lights[l];
        r.light_type = l == 0 ? 2u : 1u, r.shadow_data_index = l == 0 ? 0xFFFFFFFFu : BASE + l - 1u;
        r.color[0] = 1.0f, r.color[1] = 0.5f, r.color[2] = 0.25f, r.intensity = 2.0f + (float)l;
        r.position[1] = 1.5f, r.inner_radius = 0.3f, r.outer_radius = 20.0f;
        r.direction[0] = l == 1 ? 0.6f : -0.6f, r.direction[1] = 0.8f;
    }
    for (uint32_t r = 0; r < ROWS; r++)
        for (uint32_t c = 0; c < 4; c++) {
            // cascade 0 holds nothing (c.w = 0); the others map x in [-1, 0.8] and z in [0, 0.8] onto ndc [-1.4, 1.4]: only
            // cascade 3, whose scale is half, holds every pixel
            float *m = rows[r].light_projection_matrices[c];
            const float scale = c == 3 ? 0.7f : 1.4f;
            m[0] = scale / 0.9f, m[12] = 0.1f * scale / 0.9f, m[9] = scale / 0.4f, m[13] = -scale, m[6] = 0.25f, m[14] = 0.5f, m[15] = c == 0 ? 0.0f : 1.0f;
            rows[r].shadow_map_world_sizes[c] = r == 0 ? 1.0f : 0.5f;
            rows[r].shadow_map_indices[c] = (r + c) % MAPS;
        }
    for (uint32_t i = 0; i < MAPS * RES * RES; i++) maps[i] = (float)((i * 7u) % 11u) / 10.0f; // 0 .. 1: blockers and lit texels
    list[0] = (uint32_t)capacity;
    for (size_t c = 0; c < clusters; c++) {
        image[2 * c] = (uint32_t)(c * 3), image[2 * c + 1] = 3u;
        for (uint32_t i = 0; i < 3; i++) list[1 + c * 3 + i] = (uint32_t)((c + i) % LIGHTS);
    }
    std::vector<uint64_t> vis(W * H);
    std::vector<float> world_pos(4 * W * H), normal(3 * W * H);
    std::vector<uint32_t> material(W * H);
    const float d = 0.05f; // slice 0 with z_near 0.1, z_scale 1, z_bias -0.5: uint(log2(2) - 0.5)
    uint32_t bits;
    std::memcpy(&bits, &d, 4);
    for (uint32_t p = 0; p < W * H; p++) {
        vis[p] = p % 11 == 10 ? 0ull : ((uint64_t)bits << 32) | (p + 1u) << 8;
        world_pos[4 * p] = 0.1f * (float)(p % W) - 1.0f, world_pos[4 * p + 1] = 0.0f, world_pos[4 * p + 2] = 0.1f * (float)(p / W), world_pos[4 * p + 3] = 1.0f;
        normal[3 * p] = 0.0f, normal[3 * p + 1] = 1.0f, normal[3 * p + 2] = 0.0f;
        material[p] = p % MATERIALS;
    }
    for (int run = 0; run < 4; run++) {
        const bool tampered = run & 1;
        if (tampered) {
            lights[1].shadow_data_index = BASE + ROWS; // r = shadow_count
            rows[1].shadow_map_indices[3] = MAPS;      // map = shadow_map_count, for the pixels cascade 3 holds
        }
        std::vector<float> color(4 * W * H), factor(W * H);
        std::vector<uint32_t> walked(W * H), cascade(W * H);
        OrbitShadeStats st;
        OrbitShadowStats sh;
        OrbitFragmentsShadeShadowed j{};
        OrbitFragmentsShade &f = j.shade;
        f.visibility = vis.data(), f.world_pos = world_pos.data(), f.normal = normal.data(), f.material = material.data();
        f.materials = materials, f.lights = lights, f.cluster_offset_image = image, f.light_index_buffer = list;
        f.color = color.data(), f.lights_walked = walked.data(), f.stats = &st;
        f.material_count = MATERIALS, f.light_count = LIGHTS, f.index_capacity = (uint32_t)capacity;
        f.cluster_count[0] = CX, f.cluster_count[1] = CY, f.cluster_count[2] = 1, f.tile_size_px = 8;
        f.z_scale = 1.0f, f.z_bias = -0.5f, f.luminance_cutoff = 0.01f, f.z_near = 0.1f;
        f.view_pos[0] = 0.0f, f.view_pos[1] = 3.0f, f.view_pos[2] = 2.0f;
        f.render_mode = run < 2 ? 0u : 8u, f.width = W, f.height = H, f.flags = ORBIT_SHADE_CLEAR;
        j.shadows = rows, j.shadow_maps = maps, j.shadow_factor = factor.data(), j.cascade = cascade.data(), j.shadow_stats = &sh;
        j.shadow_count = ROWS, j.shadow_index_base = BASE, j.shadow_map_count = MAPS, j.shadow_resolution = RES;
        j.blocker_search_radius = 0.4f, j.normal_bias_scale = 2.0f, j.oriented_bias = -0.02f;
        int32_t status = 7;
        raster::fragments_shade_shadowed(j, &status);
        std::printf("mode %u, tampered %d: covered %u written %u stale %u unserved %u | shadowed %u no_cascade %u early_out %u evaluations %u status %d\n",
                    f.render_mode, (int)tampered, st.covered_pixels, st.written_pixels, st.stale_pixels, st.unserved_pixels, sh.shadowed_pixels,
                    sh.no_cascade_pixels, sh.early_out_pixels, sh.shadow_evaluations, status);
        if (st.covered_pixels != st.written_pixels + st.unshaded_pixels + st.stale_pixels || st.covered_pixels == 0) return 1;
        if (!tampered && (st.written_pixels != st.covered_pixels || status != ORBIT_OK || st.unserved_pixels != 0)) return 1;
        if (!tampered && f.render_mode == 0u && (sh.shadowed_pixels != st.written_pixels || sh.shadow_evaluations != 2 * sh.shadowed_pixels ||
                                                 sh.early_out_pixels == sh.shadowed_pixels))
            return 1;
        if (tampered && (st.stale_pixels != st.covered_pixels || status != ORBIT_E_RANGE)) return 1;
        if (tampered) { // below the base: wraps to a row far beyond shadow_count
            lights[1].shadow_data_index = BASE - 1u;
            raster::fragments_shade_shadowed(j, &status);
            if (st.stale_pixels != st.covered_pixels) return 1;
            lights[1].shadow_data_index = BASE;
            raster::fragments_shade_shadowed(j, &status); // only the map index is left: stale where cascade 3 holds the pixel, in mode 0
            if (f.render_mode == 0u ? st.stale_pixels == 0 : st.stale_pixels != 0) return 1;
            rows[1].shadow_map_indices[3] = (1 + 3) % MAPS;
        }
    }
    std::free(materials), std::free(lights), std::free(rows), std::free(maps), std::free(image), std::free(list);
    return 0;
}
