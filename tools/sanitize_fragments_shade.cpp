// sanitize_fragments_shade.cpp — the host mirror of orbit_fragments_shade (orbit_amd/host/orbit_raster.cpp over
// csrc/shade_common.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host program: a 19 x 9
// target of hand-built planes over a 3 x 2 x 4 cluster grid of 8-px tiles, with the material table, the light table, the
// (offset, count) image and the index list each in a heap buffer that ENDS at its last legal byte, so a read past a table
// is a heap overflow; first clean, then tampered: a material word = material_count, a cluster whose walk ends one past
// index_capacity, an index = light_count, an unshaded word, a slice beyond the grid.  Both render modes.  Host code only;
// nothing of it runs on a device or inside Python.  From the repository root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iorbit_amd/host tools/sanitize_fragments_shade.cpp orbit_amd/host/orbit_raster.cpp -o /tmp/sanitize_fragments_shade \
//       && /tmp/sanitize_fragments_shade
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
    const uint32_t W = 19, H = 9, CX = 3, CY = 2, CZ = 4, MATERIALS = 3, LIGHTS = 5, PER = 256; // PER indices per cluster
    const float z_near = 0.1f, z_scale = 1.0f, z_bias = 0.5f;                                  // slice = uint(log2(0.1 / d) + 0.5)
    const size_t clusters = CX * CY * CZ, capacity = clusters * PER;
    // every table ends at its last legal byte
    OrbitMaterialData *materials = (OrbitMaterialData *)std::malloc(MATERIALS * sizeof(OrbitMaterialData));
    OrbitLightData *lights = (OrbitLightData *)std::malloc(LIGHTS * sizeof(OrbitLightData));
    uint32_t *image = (uint32_t *)std::malloc(clusters * 8), *list = (uint32_t *)std::malloc(4 + capacity * 4);
    std::memset(materials, 0, MATERIALS * sizeof(OrbitMaterialData)), std::memset(lights, 0, LIGHTS * sizeof(OrbitLightData));
    for (uint32_t m = 0; m < MATERIALS; m++) {
        OrbitMaterialData &r = materials[m];
        r.base_color[0] = 0.8f, r.base_color[1] = 0.5f + 0.1f * (float)m, r.base_color[2] = 0.2f, r.base_color[3] = 1.0f;
        r.emissive_factor[m] = 0.1f, r.metallic_factor = 0.5f * (float)m, r.roughness_factor = 1.0f - 0.5f * (float)m;
        r.base_texture_index = r.normal_texture_index = r.metallic_roughness_texture_index = 0xFFFFFFFFu;
        r.occlusion_texture_index = 0xFFFFFFFFu, r.emissive_texture_index = m == 2 ? 7u : 0xFFFFFFFFu;
    }
    for (uint32_t l = 0; l < LIGHTS; l++) {
        OrbitLightData &r = lights[l];
        r.light_type = l == 3 ? 1u : l == 4 ? 0u : 2u, r.shadow_data_index = 0xFFFFFFFFu;
        r.color[0] = 1.0f, r.color[1] = 0.5f, r.color[2] = 0.25f, r.intensity = 2.0f + (float)l;
        r.position[0] = (float)l - 2.0f, r.position[1] = 1.5f, r.position[2] = 0.5f * (float)l;
        r.inner_radius = 0.05f, r.outer_radius = 20.0f, r.direction[1] = -1.0f;
    }
    list[0] = (uint32_t)capacity;
    for (size_t c = 0; c < clusters; c++) {
        // a count of 300 walks 256 = PER: the last cluster's walk ends with the list's last index
        image[2 * c] = (uint32_t)(c * PER), image[2 * c + 1] = c % 3 == 0 || c + 1 == clusters ? 300u : (uint32_t)(c * 7 % PER);
        for (uint32_t i = 0; i < PER; i++) list[1 + c * PER + i] = (uint32_t)((c + i) % LIGHTS);
    }
    std::vector<uint64_t> vis(W * H);
    std::vector<float> world_pos(4 * W * H), normal(3 * W * H);
    std::vector<uint32_t> material(W * H);
    for (uint32_t p = 0; p < W * H; p++) {
        const float d = 0.1f / std::exp2((float)((3u * (p % W) + p / W) % CZ) + 0.25f); // slices 0 .. 3
        uint32_t bits;
        std::memcpy(&bits, &d, 4);
        vis[p] = p % 11 == 10 ? 0ull : ((uint64_t)bits << 32) | (p + 1u) << 8;
        world_pos[4 * p] = 0.1f * (float)(p % W) - 1.0f, world_pos[4 * p + 1] = 0.0f, world_pos[4 * p + 2] = 0.1f * (float)(p / W), world_pos[4 * p + 3] = 1.0f;
        normal[3 * p] = 0.0f, normal[3 * p + 1] = 1.0f, normal[3 * p + 2] = 0.0f;
        material[p] = p % MATERIALS;
    }
    for (int run = 0; run < 4; run++) {
        const bool tampered = run & 1;
        std::vector<uint64_t> buf = vis;
        std::vector<uint32_t> mat = material;
        uint32_t index_capacity = (uint32_t)capacity;
        if (tampered) {
            mat[5] = MATERIALS;               // stale
            mat[6] = 0xFFFFFFFFu;             // unshaded
            index_capacity -= 1;              // the last cluster's walk ends one past it
            list[1 + 1 * PER + 0] = LIGHTS;   // cluster 1's first index = light_count
            const float beyond = 0.1f / 64.0f; // slice 6 >= CZ: outside
            uint32_t bits;
            std::memcpy(&bits, &beyond, 4);
            buf[7] = ((uint64_t)bits << 32) | 0x100u;
        }
        std::vector<float> color(4 * W * H);
        std::vector<uint32_t> walked(W * H);
        OrbitShadeStats st;
        OrbitFragmentsShade f{};
        f.visibility = buf.data(), f.world_pos = world_pos.data(), f.normal = normal.data(), f.material = mat.data();
        f.materials = materials, f.lights = lights, f.cluster_offset_image = image, f.light_index_buffer = list;
        f.color = color.data(), f.lights_walked = walked.data(), f.stats = &st;
        f.material_count = MATERIALS, f.light_count = LIGHTS, f.index_capacity = index_capacity;
        f.cluster_count[0] = CX, f.cluster_count[1] = CY, f.cluster_count[2] = CZ, f.tile_size_px = 8;
        f.z_scale = z_scale, f.z_bias = z_bias, f.luminance_cutoff = 0.01f, f.z_near = z_near;
        f.view_pos[0] = 0.0f, f.view_pos[1] = 3.0f, f.view_pos[2] = 2.0f;
        f.render_mode = run < 2 ? 0u : 8u, f.width = W, f.height = H, f.flags = ORBIT_SHADE_CLEAR;
        int32_t status = 7;
        raster::fragments_shade(f, &status);
        std::printf("mode %u, tampered %d: covered %u written %u unshaded %u stale %u outside %u degenerate %u textured %u unserved %u status %d\n",
                    f.render_mode, (int)tampered, st.covered_pixels, st.written_pixels, st.unshaded_pixels, st.stale_pixels, st.outside_pixels,
                    st.degenerate_pixels, st.textured_pixels, st.unserved_pixels, status);
        if (st.covered_pixels != st.written_pixels + st.unshaded_pixels + st.stale_pixels || st.covered_pixels == 0) return 1;
        if (!tampered && (st.written_pixels != st.covered_pixels || status != ORBIT_OK || st.textured_pixels == 0)) return 1;
        if (tampered && (st.stale_pixels < 3 || st.unshaded_pixels != 1 || st.outside_pixels != 1 || status != ORBIT_E_RANGE)) return 1;
        if (f.render_mode == 0u && st.unserved_pixels == 0) return 1;
        if (tampered) list[1 + 1 * PER + 0] = 1u % LIGHTS;
    }
    std::free(materials), std::free(lights), std::free(image), std::free(list);
    return 0;
}
