// orbit_ssao.cpp — see orbit_ssao.hpp.
#include "orbit_ssao.hpp"

#include <cmath>
#include <cstring>

#include "../csrc/ssao_common.h"
#include "orbit_host.hpp"

namespace orbit {
namespace raster {

namespace {

struct PlaneFetch { // a float plane as it is
    const float *plane;
    uint32_t w;
    float operator()(uint32_t ix, uint32_t iy) const { return plane[(size_t)iy * w + ix]; }
};
struct ByteFetch { // an R8_UNORM plane
    const uint8_t *plane;
    uint32_t w;
    float operator()(uint32_t ix, uint32_t iy) const { return (float)plane[(size_t)iy * w + ix] / 255.0f; }
};

void check(const OrbitSsao &j) {
    if (j.flags != 0u) throw Panic("ssao: unknown flags");
    if (j.screen_w == 0 || j.screen_h == 0 || j.screen_w > ORBIT_RASTER_MAX_DIM || j.screen_h > ORBIT_RASTER_MAX_DIM) throw Panic("ssao: screen size");
    if (j.ssao_w == 0 || j.ssao_h == 0 || j.ssao_w > j.screen_w || j.ssao_h > j.screen_h) throw Panic("ssao: ssao size");
    if (j.noise_size == 0 || j.noise_size > ORBIT_SSAO_MAX_NOISE_SIZE || j.samples_size == 0 || j.samples_size > ORBIT_SSAO_MAX_SAMPLES_SIZE)
        throw Panic("ssao: noise_size or samples_size");
    if (j.sample_count == 0 || j.sample_count > ORBIT_SSAO_MAX_SAMPLES) throw Panic("ssao: sample_count");
    for (const float v : {j.min_radius, j.max_radius})
        if (!(v >= 0.0f && v < INFINITY)) throw Panic("ssao: a radius negative or not finite");
    if (!j.depth || !j.noise || !j.samples) throw Panic("ssao: NULL input");
    if (!j.raw && !j.blurred && !j.ao_pixel) throw Panic("ssao: raw, blurred and ao_pixel are all NULL");
    if ((j.blurred && !j.raw) || (j.ao_pixel && !j.blurred)) throw Panic("ssao: blurred needs raw and ao_pixel needs blurred");
    if ((((uintptr_t)j.depth | (uintptr_t)j.ao_pixel | (uintptr_t)j.samples) & 3u) || ((uintptr_t)j.noise & 1u) || ((uintptr_t)j.stats & 7u))
        throw Panic("ssao: alignment");
    const void *const inputs[3] = {j.depth, j.noise, j.samples};
    const void *const outputs[4] = {j.raw, j.blurred, j.ao_pixel, j.stats};
    for (int a = 0; a < 4; a++) {
        for (const void *in : inputs)
            if (outputs[a] && outputs[a] == in) throw Panic("ssao: an output is an input");
        for (int b = a + 1; b < 4; b++)
            if (outputs[a] && outputs[a] == outputs[b]) throw Panic("ssao: two outputs are one buffer");
    }
}

} // namespace

void ssao(const OrbitSsao &j, uint64_t *census) {
    check(j);
    const PlaneFetch depth{j.depth, j.screen_w};
    const float rcp_w = 1.0f / (float)j.ssao_w, rcp_h = 1.0f / (float)j.ssao_h;
    float table[4u * kSsaoMaxSamples];
    ssao_table(j.samples, j.samples_size, j.sample_count, j.min_radius, j.max_radius, table);
    OrbitSsaoStats st{};
    st.pixels = j.ssao_w * j.ssao_h;
    SsaoCensus cs{};
    uint64_t branches[4] = {0, 0, 0, 0}, ties[2] = {0, 0};
    for (uint32_t y = 0; y < j.ssao_h; y++)
        for (uint32_t x = 0; x < j.ssao_w; x++) {
            const auto at = [&](uint32_t px, uint32_t py, float *p) { ssao_position(depth, j.inverse_projection, px, py, rcp_w, rcp_h, j.screen_w, j.screen_h, p); };
            float p0[3], right[3], left[3], down[3], up[3], normal[3], tangent[3], bitangent[3];
            at(x, y, p0), at(x + 1u, y, right), at(x - 1u, y, left), at(x, y + 1u, down), at(x, y - 1u, up); // x - 1u wraps, as the shader's uvec2
            uint32_t marks = ssao_normal(p0, right, left, down, up, normal);
            ssao_basis(j.noise, j.noise_size, x, y, normal, tangent, bitangent);
            uint32_t in_range;
            const float occlusion = ssao_occlusion(depth, j.projection, j.screen_w, j.screen_h, p0, tangent, bitangent, normal, table, j.sample_count,
                                                   j.min_radius, in_range, census ? &cs : nullptr);
            const uint32_t byte = ssao_pixel_byte(occlusion, j.sample_count, marks);
            j.raw[(size_t)y * j.ssao_w + x] = (uint8_t)byte;
            st.samples_in_range += in_range;
            if (marks & kSsaoNonfinite) st.nonfinite_pixels++;
            if (byte == 255u) st.unoccluded_pixels++;
            branches[marks & kSsaoBranchMask]++;
            if (marks & kSsaoTieHorizontal) ties[0]++;
            if (marks & kSsaoTieVertical) ties[1]++;
        }
    if (j.blurred)
        for (uint32_t y = 0; y < j.ssao_h; y++)
            for (uint32_t x = 0; x < j.ssao_w; x++)
                j.blurred[(size_t)y * j.ssao_w + x] = (uint8_t)ssao_blur_texel(ByteFetch{j.raw, j.ssao_w}, x, y, j.ssao_w, j.ssao_h);
    if (j.ao_pixel)
        for (uint32_t y = 0; y < j.screen_h; y++)
            for (uint32_t x = 0; x < j.screen_w; x++)
                j.ao_pixel[(size_t)y * j.screen_w + x] = ssao_pixel_read(ByteFetch{j.blurred, j.ssao_w}, x, y, j.screen_w, j.screen_h, j.ssao_w, j.ssao_h);
    if (j.stats) *j.stats = st;
    if (census) {
        const uint64_t samples = (uint64_t)st.pixels * j.sample_count;
        const uint64_t out[19] = {branches[0], branches[1], branches[2], branches[3], st.samples_in_range, samples - st.samples_in_range, cs.occluded,
                                  cs.unoccluded, cs.range_inside, cs.range_zero, cs.range_one, cs.range_nan, cs.depth_equal, ties[0], ties[1],
                                  cs.proj_at_zero, cs.proj_at_one, cs.proj_below_zero, cs.proj_above_one};
        std::memcpy(census, out, sizeof(out));
    }
}

void ssao_table(const uint8_t *samples, uint32_t samples_size, uint32_t sample_count, float min_radius, float max_radius, float *table) {
    for (uint32_t i = 0; i < sample_count; i++) ssao_table_entry(samples, samples_size, i, sample_count, min_radius, max_radius, table + 4u * i);
}
void ssao_in_range_array(const float *proj, uint64_t n, uint8_t *out) {
    for (uint64_t i = 0; i < n; i++) out[i] = ssao_in_range(proj + 3u * i) ? 1u : 0u;
}
void ssao_range_check_array(const float *args, uint64_t n, float *out) {
    for (uint64_t i = 0; i < n; i++) out[i] = ssao_range_check(args[3u * i], args[3u * i + 1u], args[3u * i + 2u]);
}

} // namespace raster
} // namespace orbit
