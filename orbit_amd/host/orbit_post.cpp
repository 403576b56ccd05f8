// orbit_post.cpp — see orbit_post.hpp.
#include "orbit_post.hpp"

#include <cmath>
#include <cstring>

#include "../csrc/post_common.h"
#include "orbit_host.hpp"

namespace orbit {
namespace raster {

namespace {

bool finite_not_negative(float v) { return v >= 0.0f && v < INFINITY; }

struct ColorFetch { // B8 of a colour plane
    const float *color;
    uint32_t w;
    void operator()(uint32_t ix, uint32_t iy, float *rgb) const { bloom_color_texel(color + 4u * ((size_t)iy * w + ix), rgb); }
};
struct PackedFetch { // B7 of a level
    const uint32_t *words;
    uint32_t w;
    void operator()(uint32_t ix, uint32_t iy, float *rgb) const { bloom_unpack(words[(size_t)iy * w + ix], rgb); }
};
struct FloatFetch { // three floats per texel, as they are
    const float *rgb3;
    uint32_t w;
    void operator()(uint32_t ix, uint32_t iy, float *rgb) const { std::memcpy(rgb, rgb3 + 3u * ((size_t)iy * w + ix), 12); }
};

} // namespace

void bloom(const OrbitBloom &j) {
    if (j.flags & ~(ORBIT_BLOOM_FORCE_PER_LEVEL | ORBIT_BLOOM_FORCE_DIRECT)) throw Panic("bloom: unknown flags");
    if (j.width == 0 || j.height == 0 || j.width > ORBIT_RASTER_MAX_DIM || j.height > ORBIT_RASTER_MAX_DIM) throw Panic("bloom: target size");
    if (j.max_levels == 0 || j.max_levels > ORBIT_BLOOM_MAX_LEVELS) throw Panic("bloom: max_levels");
    if (!finite_not_negative(j.threshold) || !finite_not_negative(j.soft_threshold) || !finite_not_negative(j.filter_radius))
        throw Panic("bloom: threshold, soft_threshold or filter_radius negative or not finite");
    if (!j.color || !j.mips) throw Panic("bloom: NULL argument");
    if (((uintptr_t)j.color & 15u) || (((uintptr_t)j.mips | (uintptr_t)j.stats) & 3u)) throw Panic("bloom: alignment");
    if ((const void *)j.mips == (const void *)j.color) throw Panic("bloom: mips is color");
    OrbitBloomLayout lay;
    bloom_layout(j.width, j.height, j.max_levels, lay);
    OrbitBloomStats st{};
    st.levels = lay.levels;
    float tf[4];
    bloom_threshold_filter(j.threshold, j.soft_threshold, tf); // B2
    for (uint32_t k = 0; k < lay.levels; k++) {                // B1: down
        uint32_t *dst = j.mips + lay.level_offset[k];
        const uint32_t dw = lay.level_width[k], dh = lay.level_height[k];
        for (uint32_t y = 0; y < dh; y++)
            for (uint32_t x = 0; x < dw; x++) {
                float result[3];
                if (k == 0u) {
                    bloom_down_texel(ColorFetch{j.color, j.width}, j.width, j.height, dw, dh, x, y, true, tf, result);
                    float rgb[3];
                    if (!bloom_color_texel(j.color + 4u * ((size_t)y * j.width + x), rgb)) st.nonfinite_inputs++;
                } else {
                    const uint32_t sw = lay.level_width[k - 1u], sh = lay.level_height[k - 1u];
                    bloom_down_texel(PackedFetch{j.mips + lay.level_offset[k - 1u], sw}, sw, sh, dw, dh, x, y, false, tf, result);
                }
                bool clamped = false;
                dst[(size_t)y * dw + x] = bloom_pack(result, clamped);
                st.texels_written++;
                if (clamped) st.clamped_texels++;
            }
    }
    for (uint32_t k = lay.levels - 1u; k >= 1u; k--) { // B1: up, level k into level k - 1
        uint32_t *dst = j.mips + lay.level_offset[k - 1u];
        const uint32_t sw = lay.level_width[k], sh = lay.level_height[k], dw = lay.level_width[k - 1u], dh = lay.level_height[k - 1u];
        const PackedFetch fetch{j.mips + lay.level_offset[k], sw};
        for (uint32_t y = 0; y < dh; y++)
            for (uint32_t x = 0; x < dw; x++) {
                float result[3], old[3];
                bloom_up_texel(fetch, sw, sh, dw, dh, x, y, j.filter_radius, result);
                bloom_unpack(dst[(size_t)y * dw + x], old);
                for (int i = 0; i < 3; i++) result[i] = old[i] + result[i];
                bool clamped = false;
                dst[(size_t)y * dw + x] = bloom_pack(result, clamped);
                st.texels_written++;
                if (clamped) st.clamped_texels++;
            }
    }
    if (j.stats) *j.stats = st;
}

void post_process(const OrbitPostProcess &j) {
    if (j.flags & ~ORBIT_POST_BGRA) throw Panic("post_process: unknown flags");
    if (j.render_mode != 0u && j.render_mode != 8u) throw Panic("post_process: render_mode");
    if (j.width == 0 || j.height == 0 || j.width > ORBIT_RASTER_MAX_DIM || j.height > ORBIT_RASTER_MAX_DIM) throw Panic("post_process: target size");
    if (!(std::fabs(j.exposure) < INFINITY) || !(std::fabs(j.bloom_intensity) < INFINITY)) throw Panic("post_process: exposure or bloom_intensity not finite");
    if (!j.color) throw Panic("post_process: color is NULL");
    if (!j.ldr && !j.rgba8) throw Panic("post_process: ldr and rgba8 are both NULL");
    if ((((uintptr_t)j.color | (uintptr_t)j.ldr) & 15u) || (((uintptr_t)j.bloom | (uintptr_t)j.rgba8 | (uintptr_t)j.stats) & 3u))
        throw Panic("post_process: alignment");
    const void *const inputs[2] = {j.color, j.bloom};
    const void *const outputs[3] = {j.ldr, j.rgba8, j.stats};
    for (int a = 0; a < 3; a++) {
        for (const void *in : inputs)
            if (outputs[a] && outputs[a] == in) throw Panic("post_process: an output is an input");
        for (int b = a + 1; b < 3; b++)
            if (outputs[a] && outputs[a] == outputs[b]) throw Panic("post_process: two outputs are one buffer");
    }
    const size_t pixels = (size_t)j.width * j.height;
    const bool with_bloom = j.render_mode == 0u && j.bloom != nullptr, bgra = (j.flags & ORBIT_POST_BGRA) != 0u;
    OrbitPostStats st{};
    st.pixels = (uint32_t)pixels;
    for (size_t p = 0; p < pixels; p++) {
        float ldr[4];
        uint32_t rgba8;
        const uint32_t marks = post_pixel(j.color + 4u * p, with_bloom, with_bloom ? j.bloom[p] : 0u, j.exposure, j.bloom_intensity, bgra, ldr, rgba8);
        if (marks & kPostNonfinite) st.nonfinite_pixels++;
        if (marks & kPostBloom) st.bloom_pixels++;
        if (j.ldr) std::memcpy(j.ldr + 4u * p, ldr, 16);
        if (j.rgba8) std::memcpy(j.rgba8 + 4u * p, &rgba8, 4);
    }
    if (j.stats) *j.stats = st;
}

void bloom_downsample_floats(const float *src, uint32_t src_w, uint32_t src_h, uint32_t dst_w, uint32_t dst_h, bool level0,
                             const float *tf, float *dst) {
    const float none[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t y = 0; y < dst_h; y++)
        for (uint32_t x = 0; x < dst_w; x++)
            bloom_down_texel(FloatFetch{src, src_w}, src_w, src_h, dst_w, dst_h, x, y, level0, tf ? tf : none, dst + 3u * ((size_t)y * dst_w + x));
}

void bloom_upsample_floats(const float *src, uint32_t src_w, uint32_t src_h, uint32_t dst_w, uint32_t dst_h, float filter_radius,
                           float *dst) {
    for (uint32_t y = 0; y < dst_h; y++)
        for (uint32_t x = 0; x < dst_w; x++)
            bloom_up_texel(FloatFetch{src, src_w}, src_w, src_h, dst_w, dst_h, x, y, filter_radius, dst + 3u * ((size_t)y * dst_w + x));
}

void bloom_pack_texels(const float *rgb, uint64_t n, uint32_t *words, uint8_t *clamped) {
    for (uint64_t i = 0; i < n; i++) {
        bool c = false;
        words[i] = bloom_pack(rgb + 3u * i, c);
        if (clamped) clamped[i] = c ? 1u : 0u;
    }
}
void bloom_unpack_texels(const uint32_t *words, uint64_t n, float *rgb) {
    for (uint64_t i = 0; i < n; i++) bloom_unpack(words[i], rgb + 3u * i);
}
void powc_array(const float *x, uint64_t n, float y, float *out) {
    for (uint64_t i = 0; i < n; i++) out[i] = post_powc(x[i], y);
}

} // namespace raster
} // namespace orbit
